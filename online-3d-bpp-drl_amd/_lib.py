"""ctypes binding of libbpp_hip.so (include/bpp_abi.h) -- the only way the package reaches the kernels.

There is deliberately NO fallback: if the HIP library cannot be built/loaded, or a call fails, a
RuntimeError is raised.  The CPU oracle under oracle/ is never imported from here.
"""
import ctypes
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "bpp_kernels.hip")
# build() only ever writes BUILD_LIB.  BPP_HIP_LIB: LOAD another build of the same library instead (profiling /
# diagnostic builds of tools/build_variant.sh abl -DBPP_ENABLE_ABLATION, tools/stress_stats.py) -- never built to, never a fallback
BUILD_LIB = os.path.join(CSRC, "libbpp_hip.so")
LIB = os.environ.get("BPP_HIP_LIB") or BUILD_LIB
HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_abi.h")
BRANCH_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_branch.h")
REORDER_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_reorder.h")
MULTIBIN_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_multibin.h")
MCTS_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_mcts.h")
PIPELINE_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_pipeline.h")
ROLLOUT_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_rollout.h")
UPDATE_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_update.h")
KFAC_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_kfac.h")
POLICY_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_policy.h")
STREAM_KINDS_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_stream_kinds.h")
PLACEMENTS_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_placements.h")
# everything a rebuild depends on, by glob: a new .inl or header counts from the moment it exists
DEPS = sorted(f for d, pats in ((CSRC, ("*.hip", "*.inl")), (os.path.dirname(HDR), ("*.h", "*.inl")))
              for pat in pats for f in glob.glob(os.path.join(d, pat)))

ABI_VERSION = 16
STREAM_RNG_MT19937, STREAM_RNG_COUNTER = 0, 1
RULE_UTILS, RULE_SPACE = 0, 1
RESET_INIT, RESET_ADVANCE = 0, 1
REDUCE_LANES = 1024
REDUCE_SCRATCH_BYTES = REDUCE_LANES * 4 * 8 + 64

SYMBOLS = ["bpp_abi_version", "bpp_last_error", "bpp_limits", "bpp_reset", "bpp_step", "bpp_mask_from_obs",
           "bpp_mask_from_hmap", "bpp_sample_feasible", "bpp_episode_stats", "bpp_rollout_uniform", "bpp_masked_act", "bpp_gen_cut2", "bpp_gen_cut1", "bpp_gen_rs",
           "bpp_get_knobs", "bpp_set_knobs", "bpp_launch_info", "bpp_stream_sizes", "bpp_stream_init", "bpp_stream_refill",
           "bpp_rollout_uniform_stream", "bpp_masked_evaluate", "bpp_masked_evaluate_backward", "bpp_episode_acc_reduce", "bpp_rollout_uniform_sets", "bpp_fetch_to_host", "bpp_wait", "bpp_gather_finished", "bpp_epsilon_override", "bpp_side_create", "bpp_side_destroy", "bpp_mark", "bpp_wait_mark", "bpp_step_dropin", "bpp_masked_act_counter"]
# include/bpp_branch.h: exported by libbpp_hip.so only (not part of bpp_abi.h, which the oracle library implements too)
BRANCH_SYMBOLS = ["bpp_step_subset", "bpp_copy_bins"]
# include/bpp_reorder.h: the same, for the BPP-k reorder search
REORDER_SYMBOLS = ["bpp_reorder_sizes", "bpp_reorder_begin", "bpp_reorder_emit", "bpp_reorder_choose", "bpp_reorder_commit",
                   "bpp_reorder_finish"]
REORDER_MAX_K = 8
# include/bpp_multibin.h: the same, for multi-bin packing
MULTIBIN_SYMBOLS = ["bpp_multibin_sizes", "bpp_multibin_emit", "bpp_multibin_choose", "bpp_multibin_commit", "bpp_multibin_clear"]
MULTIBIN_MAX_K = 256
# include/bpp_mcts.h: the same, for the batched MCTS
MCTS_SYMBOLS = ["bpp_mcts_sizes", "bpp_mcts_seed", "bpp_mcts_clear", "bpp_mcts_begin", "bpp_mcts_select", "bpp_mcts_emit",
                "bpp_mcts_expand", "bpp_mcts_rollout", "bpp_mcts_backup", "bpp_mcts_finish", "bpp_mcts_advance"]
MCTS_MAX_K = 16
# include/bpp_pipeline.h: the same, for the pipelined rollout driver
PIPELINE_SYMBOLS = ["bpp_pipeline_create", "bpp_pipeline_destroy", "bpp_pipeline_plan", "bpp_rollout_uniform_sets_pipelined"]
PIPELINE_MAX_GROUPS, PIPELINE_ALIGN, PIPELINE_MIN_GROUP = 4, 64, 8192
# include/bpp_rollout.h: the same, for the returns of a device-resident rollout storage
ROLLOUT_SYMBOLS = ["bpp_compute_returns", "bpp_compute_returns_host", "bpp_compute_returns_info"]
# include/bpp_update.h: the same, for the fused loss of the A2C update
UPDATE_SYMBOLS = ["bpp_a2c_loss", "bpp_a2c_loss_workspace", "bpp_a2c_loss_info"]
A2C_TERMS = ("value_loss", "action_loss", "dist_entropy", "prob_loss", "graph_loss", "loss")
# include/bpp_ppo.h: the same, for the PPO update (advantages, mini-batch gather, clipped loss)
PPO_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_ppo.h")
PPO_SYMBOLS = ["bpp_ppo_advantages", "bpp_ppo_advantages_workspace", "bpp_ppo_advantages_info", "bpp_gather_rows", "bpp_ppo_loss",
               "bpp_ppo_loss_workspace", "bpp_ppo_loss_info"]
PPO_TERMS = ("value_loss", "action_loss", "dist_entropy", "prob_loss", "graph_loss", "loss", "clip_fraction")
PPO_ROWS = ("value_term", "action_term", "entropy", "bad", "sq", "ratio", "clipped")
# include/bpp_kfac.h: the same, for the Kronecker factors of K-FAC
KFAC_SYMBOLS = ["bpp_kfac_factor", "bpp_kfac_factor_workspace", "bpp_kfac_factor_info"]
KFAC_PATCH, KFAC_ROWS, KFAC_NCHW = 0, 1, 2
KFAC_INFO = ("D", "R", "tile", "rows_per_split", "splits", "chain")
# include/bpp_policy.h: the same, for the CNNPro policy forward
POLICY_SYMBOLS = ["bpp_policy_forward", "bpp_policy_forward_workspace", "bpp_policy_weights_floats", "bpp_policy_forward_info"]
POLICY_INFO = ("bins_per_trunk_group", "trunk_lds_bytes", "trunk_groups", "bins_per_head_tile", "head_groups", "tile", "padded_rows", "path")
# include/bpp_policy_one_image.h: the same, for the policy forward on one LDS image per bin (sides up to 22)
POLICY_ONE_IMAGE_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_policy_one_image.h")
POLICY_ONE_IMAGE_SYMBOLS = ["bpp_policy_forward_one_image", "bpp_policy_forward_one_image_workspace", "bpp_policy_one_image_weights_floats",
                            "bpp_policy_forward_one_image_info"]
POLICY_ONE_IMAGE_INFO = ("bins_per_trunk_group", "trunk_lds_bytes", "trunk_groups", "tiles_per_wave", "head_groups", "tile", "padded_rows", "path")
# the forms of the policy forward: name -> ((forward, workspace, weights floats, info) symbols, the info names, the largest side)
POLICY_FORMS = {"two_images": (POLICY_SYMBOLS, POLICY_INFO, 15), "one_image": (POLICY_ONE_IMAGE_SYMBOLS, POLICY_ONE_IMAGE_INFO, 22)}
# include/bpp_policy_train.h: the same, for the training pass of the CNNPro trunk
POLICY_TRAIN_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_policy_train.h")
POLICY_TRAIN_SYMBOLS = ["bpp_policy_trunk_forward_train", "bpp_policy_trunk_backward", "bpp_policy_trunk_backward_workspace",
                        "bpp_policy_trunk_backward_weights_floats", "bpp_policy_trunk_backward_info"]
POLICY_TRAIN_INFO = ("bins_per_group", "grad_lds_bytes", "bins_per_split", "splits", "chain_rows", "wgrad_lds_bytes", "path", "blocks")
POLICY_TRUNK_FLOATS, POLICY_TRUNK_BWD_FLOATS = 151380, 148736
# include/bpp_policy_heads_train.h: the same, for the training pass of the heads' six Linear layers
POLICY_HEADS_TRAIN_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_policy_heads_train.h")
POLICY_HEADS_TRAIN_SYMBOLS = ["bpp_policy_heads_forward_train", "bpp_policy_heads_backward", "bpp_policy_heads_backward_workspace",
                              "bpp_policy_heads_backward_weights_floats", "bpp_policy_heads_backward_info"]
POLICY_HEADS_TRAIN_INFO = ("bins_per_group", "grad_lds_bytes", "bins_per_split", "splits", "chain_rows", "wgrad_lds_bytes", "path", "blocks")
# include/bpp_stream_kinds.h: the same, for the CUT-1 and RS ring refills
STREAM_KIND_SYMBOLS = ["bpp_stream_refill_cut1", "bpp_stream_refill_rs", "bpp_stream_kinds_info", "bpp_rollout_uniform_stream_kind"]
STREAM_KINDS = {"cut1": 1, "rs": 2}                  # BPP_STREAM_KIND_*
CUT1_MAX_PIECES, RS_MAX_SET = 128, 4096
STREAM_KINDS_INFO = ("lanes", "lds_bytes", "pieces", "threads")
# include/bpp_placements.h: the same, for the recorded packing plans
PLACEMENT_SYMBOLS = ["bpp_placements_sizes", "bpp_placements_clear", "bpp_placements_note", "bpp_placements_commit", "bpp_placements_copy",
                     "bpp_placements_gather", "bpp_placements_replay", "bpp_placements_info"]
PLAN_RUNNING, PLAN_FINISHED = 0, 1                   # BPP_PLAN_*
PLACEMENT_BYTES, PLACEMENTS_MAX_CAPACITY = 8, 1 << 20
PLACEMENTS_INFO = ("step_lanes", "step_groups", "plan_waves", "plan_groups", "replay_cells_per_lane", "record_bytes")
# include/bpp_heuristic.h: the same, for the lowest-top packing heuristic
HEURISTIC_HDR = os.path.join(os.path.dirname(HERE), "include", "bpp_heuristic.h")
HEURISTIC_SYMBOLS = ["bpp_heuristic_act", "bpp_heuristic_act_info"]
HEURISTIC_RULES = {"lowest_top": 0, "lowest_top_plain": 1}      # BPP_HEUR_*
HEURISTIC_INFO = ("bins_per_wave", "lds_bytes", "workgroups", "path")


class Batch(ctypes.Structure):
    """struct bpp_batch"""
    _fields_ = [("num_envs", ctypes.c_int32), ("W", ctypes.c_int32), ("L", ctypes.c_int32), ("H", ctypes.c_int32),
                ("rotation", ctypes.c_int32), ("mask_rule", ctypes.c_int32), ("pool_size", ctypes.c_int32),
                ("pool_len", ctypes.c_int32), ("env_id_base", ctypes.c_int64), ("env_id_total", ctypes.c_int64),
                ("seq_pool", ctypes.c_void_p), ("hmap", ctypes.c_void_p), ("state", ctypes.c_void_p),
                ("ep_acc", ctypes.c_void_p), ("pool_mode", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("seq_cache", ctypes.c_void_p)]


class Stream(ctypes.Structure):
    """struct bpp_stream"""
    _fields_ = [("num_envs", ctypes.c_int32), ("depth", ctypes.c_int32), ("pool_len", ctypes.c_int32), ("W", ctypes.c_int32),
                ("L", ctypes.c_int32), ("H", ctypes.c_int32), ("bound_lo", ctypes.c_int32), ("bound_hi", ctypes.c_int32),
                ("env_id_base", ctypes.c_int64), ("seed0", ctypes.c_uint64), ("ring", ctypes.c_void_p), ("mt", ctypes.c_void_p),
                ("work", ctypes.c_void_p), ("gen_next", ctypes.c_void_p), ("state", ctypes.c_void_p), ("overflow", ctypes.c_void_p),
                ("rng", ctypes.c_int32), ("reserved1", ctypes.c_int32)]


POOL_STATIC, POOL_RING = 0, 1
SEQ_CACHE_BYTES_PER_BIN = 2 * 128 + 8 + 8   # BPP_SEQ_CACHE_BYTES(E) / E
ROLLOUT_CONTINUE = 1


def eps_q24(eps):
    """epsilon as the 24-bit fraction bpp_epsilon_override takes"""
    q24 = int(round(float(eps) * (1 << 24)))
    if not 0 <= q24 <= 1 << 24:
        raise ValueError("epsilon must be in [0, 1]")
    return q24


def rollout_eps_flags(eps):
    """BPP_ROLLOUT_EPS(q24): the flags bits of bpp_rollout_uniform_sets that carry epsilon, as the int32 the ABI takes"""
    v = (min(eps_q24(eps), (1 << 24) - 1) << 8) & 0xFFFFFFFF      # the field holds 24 bits: eps = 1.0 is clamped, not wrapped to 0
    return v - (1 << 32) if v & 0x80000000 else v


class StepOut(ctypes.Structure):
    """struct bpp_step_out"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("obs", "mask", "reward", "done", "counter", "ratio", "ep_ret", "ep_len",
                                               "next_action")] + [("sample_seed", ctypes.c_uint64),
                                                                  ("sample_step", ctypes.c_uint64),
                                                                  ("host_reward", ctypes.c_void_p), ("host_done", ctypes.c_void_p)]


class Knobs(ctypes.Structure):
    """struct bpp_knobs"""
    _fields_ = [("bins_per_wave", ctypes.c_int32), ("waves_per_group", ctypes.c_int32), ("xcd_remap", ctypes.c_int32),
                ("force_generic", ctypes.c_int32), ("ablate", ctypes.c_int32), ("legacy_fast", ctypes.c_int32),
                ("tile_groups", ctypes.c_int32), ("stream_legacy", ctypes.c_int32), ("stream_overlap", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def bind_branch(L, batch=None, step_out=None, stream=None):
    """Argument types of the BRANCH_SYMBOLS on library handle L (`batch`, `step_out`, `stream`: the ctypes classes of struct
    bpp_batch, bpp_step_out and bpp_stream)."""
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_step_subset.argtypes = [ctypes.POINTER(batch or Batch), vp, i32, vp, ctypes.POINTER(step_out or StepOut), vp, vp]
    L.bpp_copy_bins.argtypes = [ctypes.POINTER(batch or Batch), ctypes.POINTER(stream or Stream), vp, vp, i32, vp]
    for name in BRANCH_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


class Reorder(ctypes.Structure):
    """struct bpp_reorder"""
    _fields_ = [("n", ctypes.c_int32), ("k", ctypes.c_int32), ("times", ctypes.c_int32), ("max_nodes", ctypes.c_int32),
                ("v_bound", ctypes.c_double), ("ids", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("work", ctypes.c_void_p),
                ("overflow", ctypes.c_void_p), ("reserved", ctypes.c_int32)]


def bind_reorder(L, batch=None):
    """Argument types of the REORDER_SYMBOLS on library handle L (`batch`: the ctypes class of struct bpp_batch)."""
    B = ctypes.POINTER(batch or Batch)
    R = ctypes.POINTER(Reorder)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_reorder_sizes.argtypes = [i32] * 5 + [ctypes.POINTER(ctypes.c_int64)]
    L.bpp_reorder_begin.argtypes = [B, R, vp]
    L.bpp_reorder_emit.argtypes = [B, R, i32, i32, vp, vp, vp]
    L.bpp_reorder_choose.argtypes = [B, R, vp, vp, vp, vp, vp]
    L.bpp_reorder_commit.argtypes = [B, R, vp, vp]
    L.bpp_reorder_finish.argtypes = [B, R, vp, vp, vp, vp]
    for name in REORDER_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


class MultiBin(ctypes.Structure):
    """struct bpp_multibin"""
    _fields_ = [("n", ctypes.c_int32), ("w", ctypes.c_int32), ("s", ctypes.c_int32), ("K", ctypes.c_int32), ("ids", ctypes.c_void_p),
                ("state", ctypes.c_void_p), ("work", ctypes.c_void_p)]


def bind_multibin(L, batch=None):
    """Argument types of the MULTIBIN_SYMBOLS on library handle L (`batch`: the ctypes class of struct bpp_batch)."""
    B = ctypes.POINTER(batch or Batch)
    M = ctypes.POINTER(MultiBin)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_multibin_sizes.argtypes = [i32] * 6 + [ctypes.POINTER(ctypes.c_int64)]
    L.bpp_multibin_emit.argtypes = [B, M, vp, vp]
    L.bpp_multibin_choose.argtypes = [B, M, vp, vp, vp, vp, vp, vp]
    L.bpp_multibin_commit.argtypes = [B, M, vp, vp]
    L.bpp_multibin_clear.argtypes = [B, M, vp, i32, vp]
    for name in MULTIBIN_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


class Mcts(ctypes.Structure):
    """struct bpp_mcts"""
    _fields_ = [("n", ctypes.c_int32), ("k", ctypes.c_int32), ("sim_times", ctypes.c_int32), ("max_depth", ctypes.c_int32),
                ("rollout_length", ctypes.c_int32), ("cap", ctypes.c_int32), ("credit", ctypes.c_double), ("zeta", ctypes.c_double),
                ("ids", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("state", ctypes.c_void_p), ("overflow", ctypes.c_void_p),
                ("reserved", ctypes.c_int32)]


def bind_mcts(L, batch=None):
    """Argument types of the MCTS_SYMBOLS on library handle L (`batch`: the ctypes class of struct bpp_batch)."""
    B = ctypes.POINTER(batch or Batch)
    M = ctypes.POINTER(Mcts)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_mcts_sizes.argtypes = [i32] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    L.bpp_mcts_seed.argtypes = [B, M, vp, vp, i32, vp]
    L.bpp_mcts_clear.argtypes = [B, M, vp, i32, vp]
    L.bpp_mcts_begin.argtypes = [B, M, vp]
    L.bpp_mcts_select.argtypes = [B, M, i32, vp, vp, vp]
    L.bpp_mcts_emit.argtypes = [B, M, i32, vp, vp, vp]
    L.bpp_mcts_expand.argtypes = [B, M, vp, vp, vp, vp]
    L.bpp_mcts_rollout.argtypes = [B, M, vp, vp, vp, vp]
    L.bpp_mcts_backup.argtypes = [B, M, vp, vp]
    L.bpp_mcts_finish.argtypes = [B, M, vp, vp, vp]
    L.bpp_mcts_advance.argtypes = [B, M, vp, vp]
    for name in MCTS_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


def bind_rollout(L):
    """Argument types of the ROLLOUT_SYMBOLS on library handle L."""
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    L.bpp_compute_returns_host.argtypes = [vp] * 8 + [i32] * 4 + [f64, f64]
    L.bpp_compute_returns.argtypes = L.bpp_compute_returns_host.argtypes + [vp]
    L.bpp_compute_returns_info.argtypes = L.bpp_compute_returns_host.argtypes + [ctypes.POINTER(i32)]
    for name in ROLLOUT_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


def bind_update(L):
    """Argument types of the UPDATE_SYMBOLS on library handle L."""
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    L.bpp_a2c_loss.argtypes = [vp] * 6 + [f64] * 4 + [vp] * 6 + [i32, i32, vp]
    L.bpp_a2c_loss.restype = ctypes.c_int
    L.bpp_a2c_loss_workspace.argtypes = [i32, i32]
    L.bpp_a2c_loss_workspace.restype = ctypes.c_size_t
    L.bpp_a2c_loss_info.argtypes = [i32, i32, ctypes.POINTER(i32)]
    L.bpp_a2c_loss_info.restype = ctypes.c_int
    return L


def bind_ppo(L):
    """Argument types of the PPO_SYMBOLS on library handle L."""
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    L.bpp_ppo_advantages.argtypes = [vp] * 4 + [i32, vp, vp]
    L.bpp_ppo_advantages.restype = ctypes.c_int
    L.bpp_ppo_advantages_workspace.argtypes = [i32]
    L.bpp_ppo_advantages_workspace.restype = ctypes.c_size_t
    L.bpp_ppo_advantages_info.argtypes = [i32, ctypes.POINTER(i32)]
    L.bpp_ppo_advantages_info.restype = ctypes.c_int
    L.bpp_gather_rows.argtypes = [vp, i64, i64, vp, i32, i32, vp, vp]
    L.bpp_gather_rows.restype = ctypes.c_int
    L.bpp_ppo_loss.argtypes = [vp] * 10 + [f64] * 5 + [i32] + [vp] * 6 + [i32, i32, i32, vp]
    L.bpp_ppo_loss.restype = ctypes.c_int
    L.bpp_ppo_loss_workspace.argtypes = [i32, i32]
    L.bpp_ppo_loss_workspace.restype = ctypes.c_size_t
    L.bpp_ppo_loss_info.argtypes = [i32, i32, ctypes.POINTER(i32)]
    L.bpp_ppo_loss_info.restype = ctypes.c_int
    return L


def bind_kfac(L):
    """Argument types of the KFAC_SYMBOLS on library handle L."""
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    geom = ctypes.POINTER(i32)
    L.bpp_kfac_factor.argtypes = [vp, i32, geom, vp, f64, f64, i32, vp, vp]
    L.bpp_kfac_factor.restype = ctypes.c_int
    L.bpp_kfac_factor_workspace.argtypes = [i32, geom]
    L.bpp_kfac_factor_workspace.restype = ctypes.c_size_t
    L.bpp_kfac_factor_info.argtypes = [i32, geom, geom]
    L.bpp_kfac_factor_info.restype = ctypes.c_int
    return L


def bind_policy(L, form="two_images"):
    """Argument types of the four symbols of a policy-forward form (POLICY_FORMS; two images: the POLICY_SYMBOLS) on library
    handle L."""
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    geom = ctypes.POINTER(i32)
    forward, workspace, weights_floats, info = (getattr(L, name) for name in POLICY_FORMS[form][0])
    forward.argtypes, forward.restype = [vp, ctypes.c_int64, i32, geom, vp, vp, vp, vp, vp, vp], ctypes.c_int
    workspace.argtypes, workspace.restype = [geom, i32], ctypes.c_size_t
    weights_floats.argtypes, weights_floats.restype = [geom], ctypes.c_size_t
    info.argtypes, info.restype = [geom, i32, geom], ctypes.c_int
    return L


def bind_policy_one_image(L):
    """Argument types of the POLICY_ONE_IMAGE_SYMBOLS on library handle L: those of their bind_policy counterparts."""
    return bind_policy(L, "one_image")


def bind_policy_train(L):
    """Argument types of the POLICY_TRAIN_SYMBOLS on library handle L."""
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    geom = ctypes.POINTER(i32)
    L.bpp_policy_trunk_forward_train.argtypes = [vp, ctypes.c_int64, i32, geom, vp, vp, vp, vp]
    L.bpp_policy_trunk_forward_train.restype = ctypes.c_int
    L.bpp_policy_trunk_backward.argtypes = [vp, ctypes.c_int64, i32, geom] + [vp] * 7 + [ctypes.c_size_t, vp]
    L.bpp_policy_trunk_backward.restype = ctypes.c_int
    L.bpp_policy_trunk_backward_workspace.argtypes = [geom, i32]
    L.bpp_policy_trunk_backward_workspace.restype = ctypes.c_size_t
    L.bpp_policy_trunk_backward_weights_floats.argtypes = [geom]
    L.bpp_policy_trunk_backward_weights_floats.restype = ctypes.c_size_t
    L.bpp_policy_trunk_backward_info.argtypes = [geom, i32, geom]
    L.bpp_policy_trunk_backward_info.restype = ctypes.c_int
    return L


def bind_policy_heads_train(L):
    """Argument types of the POLICY_HEADS_TRAIN_SYMBOLS on library handle L."""
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    geom = ctypes.POINTER(i32)
    L.bpp_policy_heads_forward_train.argtypes = [vp, i32, geom] + [vp] * 6
    L.bpp_policy_heads_forward_train.restype = ctypes.c_int
    L.bpp_policy_heads_backward.argtypes = [vp] * 6 + [i32, geom] + [vp] * 6 + [ctypes.c_size_t, vp]
    L.bpp_policy_heads_backward.restype = ctypes.c_int
    L.bpp_policy_heads_backward_workspace.argtypes = [geom, i32]
    L.bpp_policy_heads_backward_workspace.restype = ctypes.c_size_t
    L.bpp_policy_heads_backward_weights_floats.argtypes = [geom]
    L.bpp_policy_heads_backward_weights_floats.restype = ctypes.c_size_t
    L.bpp_policy_heads_backward_info.argtypes = [geom, i32, geom]
    L.bpp_policy_heads_backward_info.restype = ctypes.c_int
    return L


def bind_stream_kinds(L, batch=None, step_out=None, stream=None):
    """Argument types of the STREAM_KIND_SYMBOLS on library handle L (`batch`, `step_out`, `stream`: the ctypes classes of struct
    bpp_batch, bpp_step_out and bpp_stream)."""
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    S, rg = ctypes.POINTER(stream or Stream), ctypes.POINTER(i32)
    L.bpp_stream_refill_cut1.argtypes = [S, rg, i32, vp]
    L.bpp_stream_refill_rs.argtypes = [S, vp, i32, vp]
    L.bpp_stream_kinds_info.argtypes = [S, i32, rg, rg]
    L.bpp_rollout_uniform_stream_kind.argtypes = [ctypes.POINTER(batch or Batch), ctypes.POINTER(step_out or StepOut), vp, u64, u64, i32, S, i32,
                                                  i32, rg, i32, vp, i32, vp]
    for name in STREAM_KIND_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


def bind_placements(L, batch=None):
    """Argument types of the PLACEMENT_SYMBOLS on library handle L (`batch`: the ctypes class of struct bpp_batch)."""
    B = ctypes.POINTER(batch or Batch)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_placements_sizes.argtypes = [i32, i32, i32]
    L.bpp_placements_sizes.restype = ctypes.c_int64
    L.bpp_placements_clear.argtypes = [vp, i32, i32, i32, vp]
    L.bpp_placements_note.argtypes = [B, vp, i32, vp, vp, i32, i32, vp]
    L.bpp_placements_commit.argtypes = [B, vp, i32, vp, vp, i32, i32, vp]
    L.bpp_placements_copy.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.bpp_placements_gather.argtypes = [vp, vp, i32, i32, vp, i32, vp, vp, i32, i32, i32, vp]
    L.bpp_placements_replay.argtypes = [vp, i32, i32, vp] + [i32] * 5 + [vp, vp, vp, vp]
    L.bpp_placements_info.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    for name in PLACEMENT_SYMBOLS[1:]:
        getattr(L, name).restype = ctypes.c_int
    return L


def bind_heuristic(L):
    """Argument types of the HEURISTIC_SYMBOLS on library handle L."""
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.bpp_heuristic_act.argtypes = [vp, ctypes.c_int64, vp] + [i32] * 5 + [vp, vp, vp]
    L.bpp_heuristic_act_info.argtypes = [i32] * 4 + [ctypes.POINTER(i32)]
    for name in HEURISTIC_SYMBOLS:
        getattr(L, name).restype = ctypes.c_int
    return L


def info_dict(fn, names, slots, *args, L=None):
    """{name: int} of what the *_info entry point `fn` (a symbol's name) of library handle L writes into its last argument,
    int32 [slots], when called with `args` in front of it."""
    out = (ctypes.c_int32 * slots)()
    check(getattr(L or lib(), fn)(*args, out), L)
    return dict(zip(names, (int(v) for v in out)))


def heuristic_info(size, rotation, n, L=None):
    """bpp_heuristic_act_info: the launch shape of the heuristic for a geometry and n bins, as a dict."""
    return info_dict("bpp_heuristic_act_info", HEURISTIC_INFO, 4, int(size[0]), int(size[1]), int(bool(rotation)), int(n), L=L)


def placements_info(E, capacity, A, L=None):
    """bpp_placements_info: the launch shapes of the plan kernels, as a dict."""
    return info_dict("bpp_placements_info", PLACEMENTS_INFO, 6, int(E), int(capacity), int(A), L=L)


def box_range_arg(box_range):
    """The box_range[6] argument of the STREAM_KIND_SYMBOLS."""
    return (ctypes.c_int32 * 6)(*[int(v) for v in box_range])


def stream_kinds_info(stream, kind, box_range=None, L=None):
    """bpp_stream_kinds_info: the form a refill of `kind` ("cut1" / "rs") takes for struct bpp_stream `stream`, as a dict."""
    return info_dict("bpp_stream_kinds_info", STREAM_KINDS_INFO, 4, ctypes.byref(stream), STREAM_KINDS[kind],
                     box_range_arg(box_range) if box_range is not None else None, L=L)


def kfac_geom(values):
    """A geom[] argument of the KFAC_SYMBOLS."""
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def build(force=False, verbose=False):
    """Compile csrc/bpp_kernels.hip for gfx950 into csrc/libbpp_hip.so (in-tree; no-op when fresh)."""
    if LIB != BUILD_LIB:        # an explicitly chosen build is loaded as it is
        if not os.path.exists(LIB):
            raise RuntimeError("BPP_HIP_LIB=%s does not exist (it is never built implicitly)" % LIB)
        return LIB

    def fresh():
        return os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS)

    if not force and fresh():
        return LIB
    import fcntl
    with open(os.path.join(CSRC, ".build.lock"), "w") as lock:      # several ranks may get here at once
        fcntl.flock(lock, fcntl.LOCK_EX)
        if force or not fresh():
            tmp = LIB + ".tmp.%d" % os.getpid()
            cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC",
                   "-shared", "-o", tmp, SRC]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            # not a fallback: the product itself gets compiled (hipcc cross-compiles without a GPU)
            try:
                build()
            except Exception as exc:  # noqa: BLE001
                raise RuntimeError("libbpp_hip.so is missing and could not be built with hipcc (%s); run "
                                   "`python -c 'import __graft_entry__ as g; g.build()'`" % (exc,))
        L = ctypes.CDLL(LIB)
        L.bpp_abi_version.restype = ctypes.c_int
        L.bpp_last_error.restype = ctypes.c_char_p
        L.bpp_limits.argtypes = [ctypes.POINTER(ctypes.c_int32)]
        L.bpp_reset.argtypes = [ctypes.POINTER(Batch), ctypes.c_int32, ctypes.POINTER(StepOut), ctypes.c_void_p]
        L.bpp_step.argtypes = [ctypes.POINTER(Batch), ctypes.c_void_p, ctypes.POINTER(StepOut), ctypes.c_void_p]
        L.bpp_mask_from_obs.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 6 + [ctypes.c_void_p]
        L.bpp_mask_from_hmap.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32] * 6 + [ctypes.c_void_p]
        L.bpp_sample_feasible.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        L.bpp_epsilon_override.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
                                           ctypes.c_uint32, ctypes.c_void_p]
        L.bpp_rollout_uniform.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(StepOut), ctypes.c_void_p, ctypes.c_uint64,
                                          ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
        L.bpp_rollout_uniform_sets.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(StepOut), ctypes.c_int32, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_void_p]
        L.bpp_masked_act.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
                                     ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
        L.bpp_masked_evaluate.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
        L.bpp_masked_evaluate_backward.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
        L.bpp_gen_cut2.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 7 + [ctypes.c_uint64, ctypes.c_int32]
        L.bpp_gen_cut1.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32,
                                                                                     ctypes.c_uint64, ctypes.c_int32]
        L.bpp_gen_rs.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64,
                                                                          ctypes.c_int32]
        L.bpp_episode_stats.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.bpp_wait.argtypes = [ctypes.c_void_p]
        L.bpp_mark.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.bpp_wait_mark.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.bpp_masked_act_counter.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_int32, ctypes.c_void_p]
        L.bpp_step_dropin.argtypes = [ctypes.POINTER(Batch), ctypes.c_void_p, ctypes.POINTER(StepOut), ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_uint32, ctypes.c_void_p]
        L.bpp_gather_finished.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        L.bpp_fetch_to_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        L.bpp_episode_acc_reduce.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        L.bpp_stream_sizes.argtypes = [ctypes.POINTER(Stream), ctypes.POINTER(ctypes.c_int64)]
        L.bpp_stream_init.argtypes = [ctypes.POINTER(Stream), ctypes.c_void_p]
        L.bpp_stream_refill.argtypes = [ctypes.POINTER(Stream), ctypes.c_void_p]
        L.bpp_rollout_uniform_stream.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(StepOut), ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_uint64, ctypes.c_int32, ctypes.POINTER(Stream), ctypes.c_int32,
                                                 ctypes.c_void_p, ctypes.c_void_p]
        L.bpp_side_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        L.bpp_side_destroy.argtypes = [ctypes.c_void_p]
        L.bpp_launch_info.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_int32)]
        L.bpp_get_knobs.argtypes = [ctypes.POINTER(Knobs)]
        L.bpp_set_knobs.argtypes = [ctypes.POINTER(Knobs)]
        L.bpp_pipeline_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32]
        L.bpp_pipeline_destroy.argtypes = [ctypes.c_void_p]
        L.bpp_pipeline_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
        L.bpp_rollout_uniform_sets_pipelined.argtypes = L.bpp_rollout_uniform_sets.argtypes[:-1] + [ctypes.c_void_p, ctypes.c_int32,
                                                                                                    ctypes.c_void_p]
        bind_branch(L)
        bind_reorder(L)
        bind_multibin(L)
        bind_mcts(L)
        bind_rollout(L)
        bind_update(L)
        bind_ppo(L)
        bind_kfac(L)
        bind_policy(L)
        bind_policy_one_image(L)
        bind_policy_train(L)
        bind_policy_heads_train(L)
        bind_stream_kinds(L)
        bind_placements(L)
        bind_heuristic(L)
        if L.bpp_abi_version() != ABI_VERSION:
            raise RuntimeError("libbpp_hip.so ABI version %d != %d" % (L.bpp_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(rc, L=None):
    """RuntimeError with bpp_last_error of library handle L (default: libbpp_hip.so) unless rc is 0."""
    if rc != 0:
        raise RuntimeError("libbpp_hip error %d: %s" % (rc, (L or lib()).bpp_last_error().decode()))


def get_knobs():
    """Current launch-shape knobs as a dict (include/bpp_abi.h: bpp_knobs)."""
    k = Knobs()
    check(lib().bpp_get_knobs(ctypes.byref(k)))
    return {n: int(getattr(k, n)) for n in ("bins_per_wave", "waves_per_group", "xcd_remap", "force_generic", "ablate", "legacy_fast", "tile_groups",
                                              "stream_legacy", "stream_overlap")}


def set_knobs(**kw):
    """Change launch-shape knobs for the whole process (results never depend on them); returns the previous
    settings so a caller can restore them: `old = set_knobs(force_generic=1); ...; set_knobs(**old)`."""
    old = get_knobs()
    new = dict(old)
    for name, v in kw.items():
        if name not in new:
            raise TypeError("unknown knob %r" % (name,))
        new[name] = int(v)
    k = Knobs(new["bins_per_wave"], new["waves_per_group"], new["xcd_remap"], new["force_generic"], new["ablate"],
              new["legacy_fast"], new["tile_groups"], new["stream_legacy"], new["stream_overlap"])
    check(lib().bpp_set_knobs(ctypes.byref(k)))
    return old


KERNEL_NAMES = {0: "bpp_kernel (cell scan)", 1: "bpp_fast_kernel (prefix image, runtime geometry)",
                2: "bpp_tile_kernel (prefix image, compile-time geometry)"}


def launch_info(E, size, rotation=False):
    """Kernel and launch shape used for a geometry under the current knobs (bpp_launch_info)."""
    out = (ctypes.c_int32 * 6)()
    check(lib().bpp_launch_info(int(E), int(size[0]), int(size[1]), int(size[2]), int(bool(rotation)), out))
    return {"kernel": int(out[0]), "kernel_name": KERNEL_NAMES.get(int(out[0]), "?"), "K": int(out[1]), "bins_per_wave": int(out[2]),
            "waves_per_group": int(out[3]), "workgroups": int(out[4]), "lds_bytes": int(out[5])}


def pipeline_plan(E, groups):
    """bpp_pipeline_plan: the [(first bin, bins)] ranges the pipelined rollout driver splits E bins into (pure host function)."""
    first, count = (ctypes.c_int32 * PIPELINE_MAX_GROUPS)(), (ctypes.c_int32 * PIPELINE_MAX_GROUPS)()
    n = lib().bpp_pipeline_plan(int(E), int(groups), first, count)
    if n < 0:
        check(n)
    return [(int(first[g]), int(count[g])) for g in range(n)]


def limits():
    out = (ctypes.c_int32 * 2)()
    check(lib().bpp_limits(out))
    return int(out[0]), int(out[1])
