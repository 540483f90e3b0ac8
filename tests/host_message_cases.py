"""The bad-argument calls behind tests/golden/host_messages.json: every host entry point of csrc/bpp_kernels.hip,
csrc/bpp_drivers.inl, csrc/bpp_update.inl and csrc/bpp_returns.inl that words its own refusals, called so that it refuses --
its NULL-pointer case and its size / alignment / mode cases; for the rollout drivers, bpp_pipeline_create, bpp_side_create,
bpp_copy_bins, bpp_step_subset and bpp_gather_finished every refusal that needs no failing HIP call.  (Not reachable on the
emulator, which has one device: "the pipe belongs to another device", "the bpp_side was created on another device".)
What is NOT recorded although it is worded the same way: bpp_debug_stamps, which exists only in builds with
-DBPP_ENABLE_ABLATION; bpp_gen_cut1's "a piece fell below the lower bound", which takes a box range the reference itself
would assert on and no input of these tests produces; and a second case of bpp_get_knobs, bpp_limits and bpp_side_create,
each of which has a single refusal that needs no failing HIP call.

collect(front) runs them on the library of a numpy front-end (oracle/oracle.py's API; tests/emu binds it to the emulated
product) and returns [[entry point, case, return code, bpp_last_error()], ...].  tests/golden/make_host_messages.py records
that list, tests/test_host_messages.py replays it: return code and text are part of what a caller sees."""
import ctypes

import numpy as np

i32, i64, u32, u64, f64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p
A = 64            # a non-NULL, 64-byte aligned address no refused call reads
NOOP_FLAGS = 0


def collect(front):
    L = ctypes.CDLL(front.LIB)        # a handle of its own: no argtypes, every argument below says its C type
    L.bpp_last_error.restype = ctypes.c_char_p
    Batch, StepOut, Stream = front.Batch, front.StepOut, front.Stream
    rows = []

    def case(entry, name, *args):
        rc = getattr(L, entry)(*args)
        assert rc != 0, (entry, name)
        rows.append([entry, name, int(rc), L.bpp_last_error().decode()])

    def batch(E=8, W=10, L_=10, H=10, rot=0, rule=0, P=4, T=12, base=0, total=None, pool=A, hmap=A, state=A, ep_acc=None, mode=0,
              cache=None):
        return ctypes.byref(Batch(E, W, L_, H, rot, rule, P, T, base, base + E if total is None else total, pool, hmap, state, ep_acc,
                                  mode, 0, cache))

    def out(obs=A, mask=A, reward=A, done=A, counter=A, ratio=A, ep_ret=A, ep_len=A, next_action=None, host_reward=None,
            host_done=None):
        return ctypes.byref(StepOut(obs, mask, reward, done, counter, ratio, ep_ret, ep_len, next_action, 0, 0, host_reward, host_done))

    def outs(*sets):
        return (StepOut * len(sets))(*[StepOut(*s) for s in sets])

    def stream(E=8, depth=8, T=40, W=10, L_=10, H=10, lo=2, hi=5, base=0, ring=A, mt=A, work=A, gen_next=A, state=A, rng=0):
        return ctypes.byref(Stream(E, depth, T, W, L_, H, lo, hi, base, 0, ring, mt, work, gen_next, state, None, rng, 0))

    p = vp(A)
    # ---- knobs, launch shape, limits
    case("bpp_get_knobs", "null", None)
    case("bpp_set_knobs", "null", None)
    case("bpp_set_knobs", "range", ctypes.byref(front.Knobs(65, 0, 1)))
    case("bpp_launch_info", "null", i32(8), i32(10), i32(10), i32(10), i32(0), None)
    case("bpp_launch_info", "size", i32(0), i32(10), i32(10), i32(10), i32(0), (i32 * 6)())
    case("bpp_launch_info", "rotation", i32(8), i32(10), i32(10), i32(10), i32(2), (i32 * 6)())
    case("bpp_launch_info", "too_large", i32(8), i32(40), i32(40), i32(10), i32(0), (i32 * 6)())
    case("bpp_limits", "null", None)
    # ---- reset / step and what fill_batch says for them
    case("bpp_reset", "null", None, i32(0), out(), None)
    case("bpp_reset", "mode", batch(), i32(2), out(), None)
    case("bpp_reset", "rule", batch(rule=5), i32(0), out(), None)
    case("bpp_step", "null", None, p, out(), None)
    case("bpp_step", "null_actions", batch(), None, out(), None)
    case("bpp_step", "next_action_without_mask", batch(), p, out(mask=None, next_action=A), None)
    case("bpp_step", "batch_null", batch(hmap=None), p, out(), None)
    case("bpp_step", "batch_empty_pool", batch(P=0), p, out(), None)
    case("bpp_step", "batch_env_id_total", batch(total=4), p, out(), None)
    case("bpp_step", "out_null", batch(), p, None, None)
    case("bpp_step", "out_null_obs", batch(), p, out(obs=None), None)
    case("bpp_step", "out_null_reward", batch(), p, out(reward=None), None)
    case("bpp_step", "out_host_pair", batch(), p, out(host_reward=A), None)
    case("bpp_step", "out_misaligned", batch(), p, out(obs=A + 8), None)
    case("bpp_step", "batch_ep_acc", batch(ep_acc=A + 16), p, out(), None)
    case("bpp_step", "ring_rows", batch(P=20, mode=1), p, out(), None)
    case("bpp_step", "ring_depth", batch(P=24, mode=1), p, out(), None)
    case("bpp_step", "ring_pool_len", batch(P=64, T=3, mode=1), p, out(), None)
    case("bpp_step", "cache_misaligned", batch(P=64, mode=1, cache=A), p, out(), None)
    case("bpp_step", "cache_depth", batch(P=32, mode=1, cache=128), p, out(), None)
    case("bpp_step", "cache_pool_len", batch(P=64, T=8192, mode=1, cache=128), p, out(), None)
    case("bpp_step", "cache_static", batch(cache=128), p, out(), None)
    case("bpp_step", "pool_mode", batch(mode=7), p, out(), None)
    sub = ("bpp_step_subset",)
    case(*sub, "null", None, p, i32(1), p, out(), None, None)
    case(*sub, "null_ids", batch(), None, i32(1), p, out(), None, None)
    case(*sub, "negative_n", batch(), p, i32(-1), p, out(), None, None)
    case(*sub, "ids_misaligned", batch(), vp(A + 4), i32(1), p, out(), None, None)
    case(*sub, "bad_ids_misaligned", batch(), p, i32(1), p, out(), vp(A + 2), None)
    case(*sub, "size", batch(E=0), p, i32(1), p, out(), None, None)
    case(*sub, "out_null_reward", batch(), p, i32(1), p, out(reward=None), None, None)
    case(*sub, "next_action_without_mask", batch(), p, i32(1), p, out(mask=None, next_action=A), None, None)
    case(*sub, "next_action_misaligned", batch(), p, i32(1), p, out(next_action=A + 4), None, None)
    # ---- masks, draws
    geo = (i32(10), i32(10), i32(10), i32(0), i32(0))
    case("bpp_mask_from_obs", "null", None, p, i32(8), *geo, None)
    case("bpp_mask_from_obs", "size", p, p, i32(-1), *geo, None)
    case("bpp_mask_from_obs", "misaligned", vp(A + 4), p, i32(8), *geo, None)
    case("bpp_mask_from_hmap", "null", p, None, p, i32(8), *geo, None)
    case("bpp_mask_from_hmap", "size", p, p, p, i32(0), *geo, None)
    case("bpp_mask_from_hmap", "misaligned", p, p, vp(A + 4), i32(8), *geo, None)
    case("bpp_sample_feasible", "null", None, p, i32(8), i32(100), i64(0), u64(1), u64(0), None)
    case("bpp_sample_feasible", "size", p, p, i32(8), i32(0), i64(0), u64(1), u64(0), None)
    case("bpp_epsilon_override", "null", None, i32(8), i32(100), i64(0), u64(1), u64(0), u32(5), None)
    case("bpp_epsilon_override", "size", p, i32(0), i32(100), i64(0), u64(1), u64(0), u32(5), None)
    case("bpp_epsilon_override", "eps", p, i32(8), i32(100), i64(0), u64(1), u64(0), u32((1 << 24) + 1), None)
    # ---- host generators
    pool = np.zeros((2, 4, 4), np.uint8)
    pp = vp(pool.ctypes.data)
    rg = (i32 * 6)(2, 2, 2, 5, 5, 5)
    case("bpp_gen_cut2", "null", None, None, i32(2), i32(40), i32(10), i32(10), i32(10), i32(2), i32(5), u64(0), i32(1))
    case("bpp_gen_cut2", "bounds", pp, None, i32(2), i32(40), i32(10), i32(10), i32(10), i32(2), i32(10), u64(0), i32(1))
    case("bpp_gen_cut2", "does_not_fit", pp, None, i32(2), i32(4), i32(10), i32(10), i32(10), i32(2), i32(5), u64(0), i32(1))
    case("bpp_gen_cut1", "null", None, None, i32(2), i32(40), i32(10), i32(10), i32(10), rg, i32(0), u64(0), i32(1))
    case("bpp_gen_cut1", "seeds", pp, None, i32(2), i32(40), i32(10), i32(10), i32(10), rg, i32(0), u64(1 << 32), i32(1))
    case("bpp_gen_cut1", "does_not_fit", pp, None, i32(2), i32(4), i32(10), i32(10), i32(10), rg, i32(0), u64(0), i32(1))
    box = (i32 * 3)(2, 3, 4)
    case("bpp_gen_rs", "null", None, i32(2), i32(4), i32(10), i32(10), i32(10), box, i32(1), u64(0), i32(1))
    case("bpp_gen_rs", "item_side", pp, i32(2), i32(4), i32(10), i32(10), i32(10), (i32 * 3)(2, 300, 4), i32(1), u64(0), i32(1))
    # ---- policy heads
    act = (i32(8), i32(100), i64(0), u64(1), u64(0), i32(0), None)
    case("bpp_masked_act", "null", None, p, p, p, *act)
    case("bpp_masked_act", "size", p, p, p, p, i32(0), *act[1:])
    ctr = (i32(8), i32(100), i64(0), p, i32(0), None)
    case("bpp_masked_act_counter", "null_seed_step", p, p, p, p, i32(8), i32(100), i64(0), None, i32(0), None)
    case("bpp_masked_act_counter", "null", p, None, p, p, *ctr)
    case("bpp_masked_act_counter", "size", p, p, p, p, i32(8), i32(-3), *ctr[2:])
    case("bpp_masked_evaluate", "null", p, p, p, p, None, p, i32(8), i32(100), None)
    case("bpp_masked_evaluate", "size", p, p, p, p, p, p, i32(0), i32(100), None)
    case("bpp_masked_evaluate_backward", "null", p, p, p, p, p, p, None, i32(8), i32(100), None)
    case("bpp_masked_evaluate_backward", "size", p, p, p, p, p, p, p, i32(8), i32(0), None)
    # ---- host transfers and marks
    case("bpp_fetch_to_host", "null", None, p, i64(8), None)
    case("bpp_fetch_to_host", "size", p, p, i64(0), None)
    g = ("bpp_gather_finished",)
    case(*g, "null", p, p, p, p, p, i32(8), None, None, i32(1), None)
    case(*g, "null_done", None, p, p, p, p, i32(8), None, p, i32(1), None)
    case(*g, "size", p, p, p, p, p, i32(0), None, p, i32(0), None)
    case(*g, "n_above_E", p, p, p, p, p, i32(8), None, p, i32(9), None)
    case(*g, "n_below_enqueue_only", p, p, p, p, p, i32(8), None, p, i32(-2), None)
    case(*g, "enqueue_only_with_dev", p, p, p, p, p, i32(8), p, p, i32(-1), None)
    case(*g, "enqueue_only_misaligned", p, p, p, p, p, i32(8), None, vp(A + 4), i32(-1), None)
    case(*g, "dev_misaligned", p, p, p, p, p, i32(8), vp(A + 4), p, i32(1), None)
    case(*g, "host_misaligned", p, p, p, p, p, i32(8), None, vp(A + 4), i32(1), None)
    done = np.array([0, 1, 0, 2, 0, 0, 1, 0], np.uint8)
    ret, ratio, ln, cnt = np.ones(8), np.ones(8), np.ones(8, np.int32), np.ones(8, np.int32)
    host = np.zeros(64, np.float64)
    case(*g, "count_of_another_step", vp(done.ctypes.data), vp(ret.ctypes.data), vp(ratio.ctypes.data), vp(ln.ctypes.data),
         vp(cnt.ctypes.data), i32(8), None, vp(host.ctypes.data), i32(2), None)
    case("bpp_mark", "null", None, u32(1), None)
    case("bpp_mark", "misaligned", vp(A + 2), u32(1), None)
    case("bpp_wait_mark", "null", None, u32(1), None)
    flag = np.zeros(1, np.uint32)
    case("bpp_wait_mark", "never_marked", vp(flag.ctypes.data), u32(1), None)
    # ---- the rollout drivers
    r = ("bpp_rollout_uniform",)
    case(*r, "null", None, out(), p, u64(1), u64(0), i32(3), None)
    case(*r, "null_out", batch(), None, p, u64(1), u64(0), i32(3), None)
    case(*r, "null_mask", batch(), out(mask=None), p, u64(1), u64(0), i32(3), None)
    case(*r, "null_actions", batch(), out(), None, u64(1), u64(0), i32(3), None)
    case(*r, "negative_nsteps", batch(), out(), p, u64(1), u64(0), i32(-1), None)
    case(*r, "size", batch(W=0), out(), p, u64(1), u64(0), i32(3), None)     # the first bpp_step's refusal
    two, tail = outs((A, A), (A, A)), (u64(1), u64(0))
    s = ("bpp_rollout_uniform_sets",)
    case(*s, "null", None, two, i32(2), p, p, *tail, i32(3), i32(0), None)
    case(*s, "null_outs", batch(), None, i32(2), p, p, *tail, i32(3), i32(0), None)
    case(*s, "null_actions", batch(), two, i32(2), p, None, *tail, i32(3), i32(0), None)
    case(*s, "no_output_set", batch(), two, i32(0), p, p, *tail, i32(3), i32(0), None)
    case(*s, "negative_nsteps", batch(), two, i32(2), p, p, *tail, i32(-1), i32(0), None)
    case(*s, "set_without_mask", batch(), outs((A, A), (A,)), i32(2), p, p, *tail, i32(3), i32(0), None)
    case(*s, "no_first_mask", batch(), two, i32(2), None, p, *tail, i32(3), i32(0), None)
    case(*s, "size", batch(W=0), two, i32(2), p, p, *tail, i32(3), i32(1), None)     # BPP_ROLLOUT_CONTINUE: the first bpp_step's refusal
    case("bpp_pipeline_plan", "null_first", i32(65536), i32(2), None, (i32 * 4)())
    case("bpp_pipeline_plan", "null_count", i32(65536), i32(2), (i32 * 4)(), None)
    case("bpp_pipeline_plan", "size", i32(0), i32(2), (i32 * 4)(), (i32 * 4)())
    case("bpp_pipeline_plan", "groups", i32(65536), i32(5), (i32 * 4)(), (i32 * 4)())
    pipe = vp()
    case("bpp_pipeline_create", "null", None, i32(2))
    case("bpp_pipeline_create", "no_group", ctypes.byref(pipe), i32(0))
    case("bpp_pipeline_create", "too_many_groups", ctypes.byref(pipe), i32(5))
    assert L.bpp_pipeline_create(ctypes.byref(pipe), i32(2)) == 0 and pipe.value
    big = 65536
    q = ("bpp_rollout_uniform_sets_pipelined",)
    host_set = outs((A, A), (A, A))
    host_set[1].host_reward, host_set[1].host_done = A, A
    case(*q, "null", None, two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "null_outs", batch(big), None, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "null_actions", batch(big), two, i32(2), p, None, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "no_output_set", batch(big), two, i32(0), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "negative_nsteps", batch(big), two, i32(2), p, p, *tail, i32(-1), i32(0), None, i32(2), None)
    case(*q, "no_group", batch(big), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(0), None)
    case(*q, "too_many_groups", batch(big), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(5), None)
    case(*q, "ring_pool", batch(big, P=8 * big, mode=1), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "row_cache", batch(big, cache=128), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "set_without_mask", batch(big), outs((A, A), (A,)), i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "host_mirrors", batch(big), host_set, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "no_first_mask", batch(big), two, i32(2), None, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "size", batch(0), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)                 # bpp_pipeline_plan's refusal
    case(*q, "no_pipe", batch(big), two, i32(2), p, p, *tail, i32(3), i32(0), None, i32(2), None)
    case(*q, "no_pipe_nsteps_0", batch(big), two, i32(2), p, p, *tail, i32(0), i32(0), None, i32(2), None)
    case(*q, "pipe_too_small", batch(big), two, i32(2), p, p, *tail, i32(3), i32(0), pipe, i32(4), None)
    case(*q, "one_group_size", batch(8, W=0), two, i32(2), p, p, *tail, i32(3), i32(1), None, i32(2), None)   # one group: bpp_step's refusal
    case(*q, "two_groups_size", batch(big, H=0), two, i32(2), p, p, *tail, i32(3), i32(1), pipe, i32(2), None)
    assert L.bpp_pipeline_destroy(pipe) == 0
    # ---- streams
    sizes = (i64 * 2)()
    case("bpp_stream_sizes", "null", None, sizes)
    case("bpp_stream_sizes", "null_out", stream(), None)
    case("bpp_stream_sizes", "depth", stream(depth=3), sizes)
    case("bpp_stream_sizes", "rng", stream(rng=2), sizes)
    for entry in ("bpp_stream_init", "bpp_stream_refill"):
        case(entry, "null", None, None)
        case(entry, "null_ring", stream(ring=None), None)
        case(entry, "depth", stream(depth=3), None)
        case(entry, "bounds", stream(hi=10), None)
        case(entry, "misaligned", stream(work=A + 8), None)
        case(entry, "rng", stream(rng=2), None)
    case("bpp_side_create", "null", None)
    ring = dict(P=64, T=40, mode=1)
    u = ("bpp_rollout_uniform_stream",)
    case(*u, "null", None, out(), p, *tail, i32(3), stream(), i32(2), None, None)
    case(*u, "null_stream", batch(**ring), out(), p, *tail, i32(3), None, i32(2), None, None)
    case(*u, "null_mask", batch(**ring), out(mask=None), p, *tail, i32(3), stream(), i32(2), None, None)
    case(*u, "null_actions", batch(**ring), out(), None, *tail, i32(3), stream(), i32(2), None, None)
    case(*u, "negative_nsteps", batch(**ring), out(), p, *tail, i32(-1), stream(), i32(2), None, None)
    case(*u, "static_pool", batch(), out(), p, *tail, i32(3), stream(), i32(2), None, None)
    case(*u, "refill_every_0", batch(**ring), out(), p, *tail, i32(3), stream(), i32(0), None, None)
    case(*u, "refill_every_above_depth", batch(**ring), out(), p, *tail, i32(3), stream(), i32(6), None, None)
    case(*u, "refill_every_above_depth_with_cache", batch(cache=128, **ring), out(), p, *tail, i32(3), stream(), i32(5), None, None)
    case(*u, "size", batch(W=0, **ring), out(), p, *tail, i32(3), stream(), i32(2), None, None)      # the first bpp_step's refusal
    # ---- statistics
    case("bpp_episode_stats", "null", p, p, p, p, i32(8), None, None)
    case("bpp_episode_stats", "size", p, p, p, p, i32(0), p, None)
    e = ("bpp_episode_acc_reduce",)
    case(*e, "null", None, i32(8), p, i32(0), None, None)
    case(*e, "size", p, i32(0), p, i32(0), None, None)
    case(*e, "ep_acc_misaligned", vp(A + 16), i32(8), p, i32(0), None, None)
    case(*e, "scratch_misaligned", p, i32(8), p, i32(0), vp(A + 4), None)
    # ---- branch copies
    c = ("bpp_copy_bins",)
    case(*c, "null", None, None, p, p, i32(1), None)
    case(*c, "null_src", batch(), None, None, p, i32(1), None)
    case(*c, "null_hmap", batch(hmap=None), None, p, p, i32(1), None)
    case(*c, "negative_n", batch(), None, p, p, i32(-1), None)
    case(*c, "size", batch(L_=0), None, p, p, i32(1), None)
    case(*c, "src_misaligned", batch(), None, vp(A + 4), p, i32(1), None)
    case(*c, "cache_misaligned", batch(cache=A, **ring), stream(), p, p, i32(1), None)
    case(*c, "ring_without_stream", batch(**ring), None, p, p, i32(1), None)
    case(*c, "stream_refused", batch(**ring), stream(depth=3), p, p, i32(1), None)
    case(*c, "stream_of_another_ring", batch(**ring), stream(ring=2 * A), p, p, i32(1), None)
    case(*c, "stream_of_another_depth", batch(P=128, T=40, mode=1), stream(), p, p, i32(1), None)
    case(*c, "static_with_stream", batch(), stream(), p, p, i32(1), None)
    case(*c, "static_with_cache", batch(cache=128), None, p, p, i32(1), None)
    case(*c, "pool_mode", batch(mode=7), None, p, p, i32(1), None)
    # ---- the A2C update's loss (csrc/bpp_update.inl)
    co = (f64(0.5), f64(0.01), f64(1.0), f64(0.5))
    case("bpp_a2c_loss_info", "size", i32(0), i32(100), (i32 * 4)())
    case("bpp_a2c_loss_info", "null", i32(8), i32(100), None)
    case("bpp_a2c_loss", "size", p, p, p, p, p, None, *co, p, p, None, None, p, p, i32(8), i32(0), None)
    case("bpp_a2c_loss", "null", p, p, p, p, p, None, *co, p, p, None, None, None, p, i32(8), i32(100), None)
    case("bpp_a2c_loss", "null_workspace", p, p, p, p, p, None, *co, p, p, None, None, p, None, i32(8), i32(100), None)
    case("bpp_a2c_loss", "pred_mask_alone", p, p, p, p, p, p, *co, p, p, None, None, p, p, i32(8), i32(100), None)
    # ---- the returns of a rollout storage (csrc/bpp_returns.inl)
    gl = (f64(0.99), f64(0.95))
    for entry, last in (("bpp_compute_returns", (None,)), ("bpp_compute_returns_info", ((i32 * 3)(),)), ("bpp_compute_returns_host", ())):
        case(entry, "size", p, p, p, p, p, None, p, None, i32(0), i32(8), i32(1), i32(0), *gl, *last)
        case(entry, "null", None, p, p, p, p, None, p, None, i32(4), i32(8), i32(1), i32(0), *gl, *last)
        case(entry, "neither_done_nor_masks", p, p, p, None, None, None, p, None, i32(4), i32(8), i32(1), i32(0), *gl, *last)
    case("bpp_compute_returns_info", "null_out", p, p, p, p, p, None, p, None, i32(4), i32(8), i32(1), i32(0), *gl, None)
    return rows
