// bpp_drivers.inl -- the rollout drivers of the benchmark policy (uniform over the feasible actions): bpp_rollout_uniform,
// bpp_rollout_uniform_sets, bpp_rollout_uniform_sets_pipelined, bpp_rollout_uniform_stream, and the caller-owned streams and events
// two of them run on (bpp_pipeline, bpp_side).  Host code only; included by bpp_kernels.hip once stream_refill is defined.
// All four enqueue the same lock-step loop, stated once in rollout_lock_steps.

namespace {

// One group of bins of a lock-step rollout: its batch, its slice of `actions`, the mask its first action is drawn from (read
// with draw_first only), the stream its launches go to and its nsets output sets, all seen from the group's first bin.
// own: the driver may write a step's draw fields into the sets themselves (the pipelined driver's per-call array); else the
// sets are the caller's and every step patches a copy on the stack.
struct RolloutGroup {
    const bpp_batch *b;
    bpp_step_out *own;
    const bpp_step_out *outs;
    int64_t *actions;
    const float *first_mask;
    void *stream;
};

// nsteps lock-steps of G groups, lock-step t into output set t % nsets.  draw_first: the action of lock-step 0 comes from first_mask
// (a standalone bpp_sample_feasible launch that reads the whole mask), else `actions` already holds it.  Every step then draws the
// next one's itself (bpp_step_out.next_action, in place), the last one only with draw_last (then `actions` holds the draw for
// lock-step step0 + nsteps and the next call needs no launch of its own for it).  eps (q24) != 0: SURVEY 8d's failure-path variant,
// one tiny bpp_epsilon_override launch behind every draw.  t-major over the groups -- lock-step t of every group, then t + 1 --
// so that all G queues hold work from the first launch on; one group: the serial order.
int rollout_lock_steps(const RolloutGroup *groups, int G, int nsets, uint64_t seed, uint64_t step0, int32_t nsteps, bool draw_first,
                       bool draw_last, uint32_t eps) {
    const int M = groups[0].b->W * groups[0].b->L * (1 + groups[0].b->rotation);
    const auto override_draw = [&](const RolloutGroup &g, uint64_t step) {
        return eps ? bpp_epsilon_override(g.actions, g.b->num_envs, M, g.b->env_id_base, seed, step, eps, g.stream) : 0;
    };
    int rc = 0;
    for (int k = 0; draw_first && rc == 0 && k < G; ++k) {
        const RolloutGroup &g = groups[k];
        rc = bpp_sample_feasible(g.first_mask, g.actions, g.b->num_envs, M, g.b->env_id_base, seed, step0, g.stream);
        if (rc == 0) rc = override_draw(g, step0);
    }
    for (int t = 0; rc == 0 && t < nsteps; ++t)
        for (int k = 0; rc == 0 && k < G; ++k) {
            const RolloutGroup &g = groups[k];
            bpp_step_out copy;
            bpp_step_out &o = g.own ? g.own[t % nsets] : (copy = g.outs[t % nsets]);
            o.next_action = (t + 1 < nsteps || draw_last) ? g.actions : nullptr;
            o.sample_seed = seed;
            o.sample_step = step0 + (uint64_t)t + 1;
            rc = bpp_step(g.b, g.actions, &o, g.stream);
            if (rc == 0 && o.next_action) rc = override_draw(g, o.sample_step);
        }
    return rc;
}

// bpp_pipeline (include/bpp_pipeline.h): the side streams and the fork / join events of the pipelined rollout driver, created and
// owned by the CALLER like bpp_side -- no per-device state in the library.
struct Pipeline {
    int device, max_groups;
    hipStream_t streams[BPP_PIPELINE_MAX_GROUPS - 1];
    hipEvent_t fork, join[BPP_PIPELINE_MAX_GROUPS - 1];
};

// bpp_side: what the overlapped schedule of bpp_rollout_uniform_stream needs beside the caller's stream -- ONE high-priority stream for
// the refills and three events -- created and owned by the CALLER (bpp_side_create / bpp_side_destroy; one per env), so that the
// library keeps no per-device state of its own (rounds 3-4 kept one lazily created set per device behind a mutex).
struct SideStream {
    hipStream_t stream;
    hipEvent_t stepped, refilled[2];
    int device;
};

// The teardowns take a partly built object too: both structs are zero-initialised on creation, a handle still null was never
// made and is skipped.  What they return is the first error of a hipStreamDestroy.
hipError_t drain_and_destroy(hipStream_t stream, hipEvent_t *events, int n) {
    if (stream) (void)hipStreamSynchronize(stream);
    for (int k = 0; k < n; ++k)
        if (events[k]) (void)hipEventDestroy(events[k]);
    return stream ? hipStreamDestroy(stream) : hipSuccess;
}

hipError_t pipeline_teardown(Pipeline *pl) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < BPP_PIPELINE_MAX_GROUPS - 1; ++k) {
        const hipError_t ek = drain_and_destroy(pl->streams[k], &pl->join[k], 1);
        if (e == hipSuccess) e = ek;
    }
    if (pl->fork) (void)hipEventDestroy(pl->fork);
    delete pl;
    return e;
}

hipError_t side_teardown(SideStream *ss) {
    hipEvent_t events[3] = {ss->stepped, ss->refilled[0], ss->refilled[1]};
    const hipError_t e = drain_and_destroy(ss->stream, events, 3);
    delete ss;
    return e;
}

template <typename T>
T *rows_from(T *p, int32_t first, size_t row) {   // NULL stays NULL
    return p ? p + (size_t)first * row : nullptr;
}

}  // namespace

extern "C" {

int bpp_rollout_uniform(const bpp_batch *b, const bpp_step_out *out, int64_t *actions, uint64_t seed, uint64_t step0,
                        int32_t nsteps, void *stream) {
    const ArgCheck ck{"bpp_rollout_uniform"};
    if (!b || !out || !out->mask || !actions) return ck.bad("NULL pointer");
    if (nsteps < 0) return ck.bad("negative nsteps");
    if (nsteps == 0) return 0;
    const RolloutGroup g{b, nullptr, out, actions, out->mask, stream};
    return rollout_lock_steps(&g, 1, 1, seed, step0, nsteps, true, false, 0);
}

int bpp_rollout_uniform_sets(const bpp_batch *b, const bpp_step_out *outs, int32_t nsets, const float *first_mask,
                             int64_t *actions, uint64_t seed, uint64_t step0, int32_t nsteps, int32_t flags, void *stream) {
    const ArgCheck ck{"bpp_rollout_uniform_sets"};
    if (!b || !outs || !actions || nsets < 1) return ck.bad("NULL pointer / no output set");
    if (nsteps < 0) return ck.bad("negative nsteps");
    for (int k = 0; k < nsets; ++k)
        if (!outs[k].mask) return ck.bad("every output set needs a mask");
    if (nsteps == 0) return 0;
    const bool draw_first = !(flags & BPP_ROLLOUT_CONTINUE);
    if (draw_first && !first_mask) return ck.bad("first_mask needed without BPP_ROLLOUT_CONTINUE");
    const RolloutGroup g{b, nullptr, outs, actions, first_mask, stream};
    return rollout_lock_steps(&g, 1, nsets, seed, step0, nsteps, draw_first, true, BPP_ROLLOUT_EPS_OF(flags));
}

int bpp_pipeline_plan(int32_t E, int32_t groups, int32_t *first, int32_t *count) {
    const ArgCheck ck{"bpp_pipeline_plan"};
    if (!first || !count) return ck.bad("NULL pointer");
    if (E <= 0 || groups < 1 || groups > BPP_PIPELINE_MAX_GROUPS) return ck.bad("need E > 0 and 1 <= groups <= BPP_PIPELINE_MAX_GROUPS");
    int n = groups;
    if (n > E / BPP_PIPELINE_MIN_GROUP) n = E / BPP_PIPELINE_MIN_GROUP;
    if (n < 1) n = 1;
    // every group but the last holds E / n bins rounded UP to the alignment; the last one takes the remainder, the smallest share --
    // where rounding up leaves it below the minimum, one group fewer is made
    for (;; --n) {
        const int64_t per = (((int64_t)E + n - 1) / n + BPP_PIPELINE_ALIGN - 1) / BPP_PIPELINE_ALIGN * BPP_PIPELINE_ALIGN;
        const int64_t last = (int64_t)E - per * (n - 1);
        if (n > 1 && last < BPP_PIPELINE_MIN_GROUP) continue;
        for (int g = 0; g < n; ++g) {
            first[g] = (int32_t)(per * g);
            count[g] = (int32_t)(g + 1 < n ? per : last);
        }
        return n;
    }
}

int bpp_pipeline_create(void **pipe, int32_t max_groups) {
    const ArgCheck ck{"bpp_pipeline_create"};
    if (!pipe) return ck.bad("NULL pointer");
    *pipe = nullptr;
    if (max_groups < 1 || max_groups > BPP_PIPELINE_MAX_GROUPS) return ck.bad("need 1 <= max_groups <= BPP_PIPELINE_MAX_GROUPS");
    Pipeline *pl = new Pipeline();
    pl->max_groups = max_groups;
    if (hipGetDevice(&pl->device) != hipSuccess) {
        (void)pipeline_teardown(pl);
        return ck.bad("no current device");
    }
    const char *what = "hipEventCreateWithFlags";
    hipError_t e = hipEventCreateWithFlags(&pl->fork, hipEventDisableTiming);
    for (int k = 0; e == hipSuccess && k < max_groups - 1; ++k) {
        what = "hipStreamCreateWithPriority";
        e = hipStreamCreateWithPriority(&pl->streams[k], hipStreamNonBlocking, 0);      // 0: the default priority
        if (e != hipSuccess) break;
        what = "hipEventCreateWithFlags";
        e = hipEventCreateWithFlags(&pl->join[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        (void)pipeline_teardown(pl);
        return hip_fail(e, what);
    }
    *pipe = pl;
    return 0;
}

int bpp_pipeline_destroy(void *pipe) {
    if (!pipe) return 0;
    const hipError_t e = pipeline_teardown((Pipeline *)pipe);
    return e == hipSuccess ? 0 : hip_fail(e, "hipStreamDestroy");
}

int bpp_rollout_uniform_sets_pipelined(const bpp_batch *b, const bpp_step_out *outs, int32_t nsets, const float *first_mask,
                                       int64_t *actions, uint64_t seed, uint64_t step0, int32_t nsteps, int32_t flags,
                                       void *pipe, int32_t groups, void *stream) {
    const ArgCheck ck{"bpp_rollout_uniform_sets_pipelined"};
    if (!b || !outs || !actions || nsets < 1) return ck.bad("NULL pointer / no output set");
    if (nsteps < 0) return ck.bad("negative nsteps");
    if (groups < 1 || groups > BPP_PIPELINE_MAX_GROUPS) return ck.bad("need 1 <= groups <= BPP_PIPELINE_MAX_GROUPS");
    if (b->pool_mode != BPP_POOL_STATIC || b->seq_cache)
        return ck.bad("static pools only (ring rows and the row cache are indexed by local bin)");
    for (int k = 0; k < nsets; ++k) {
        if (!outs[k].mask) return ck.bad("every output set needs a mask");
        if (outs[k].host_reward || outs[k].host_done) return ck.bad("output sets with host_reward / host_done are not split");
    }
    const bool draw_first = !(flags & BPP_ROLLOUT_CONTINUE);
    if (draw_first && !first_mask) return ck.bad("first_mask needed without BPP_ROLLOUT_CONTINUE");
    int32_t first[BPP_PIPELINE_MAX_GROUPS], count[BPP_PIPELINE_MAX_GROUPS];
    const int G = bpp_pipeline_plan(b->num_envs, groups, first, count);
    if (G < 0) return G;
    if (G == 1) return bpp_rollout_uniform_sets(b, outs, nsets, first_mask, actions, seed, step0, nsteps, flags, stream);
    Pipeline *pl = (Pipeline *)pipe;
    if (!pl) return ck.bad("more than one group needs a pipe (bpp_pipeline_create)");
    if (G > pl->max_groups) return ck.bad("more groups than the pipe was created for");
    if (nsteps == 0) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != pl->device) return ck.bad("the pipe belongs to another device than the current one");

    const size_t A = (size_t)b->W * b->L, M = A * (1 + b->rotation);
    bpp_batch sub[BPP_PIPELINE_MAX_GROUPS];
    RolloutGroup gr[BPP_PIPELINE_MAX_GROUPS];
    std::vector<bpp_step_out> so((size_t)G * nsets);      // [g][k]: output set k seen from group g's first bin
    for (int g = 0; g < G; ++g) {
        const int32_t f = first[g];
        sub[g] = *b;
        sub[g].num_envs = count[g];
        sub[g].env_id_base = b->env_id_base + f;
        sub[g].hmap = rows_from(b->hmap, f, A);
        sub[g].state = rows_from(b->state, f, 1);
        sub[g].ep_acc = rows_from(b->ep_acc, f, 4);
        for (int k = 0; k < nsets; ++k) {
            bpp_step_out &o = so[(size_t)g * nsets + k];
            o = outs[k];
            o.obs = rows_from(o.obs, f, 4 * A);
            o.mask = rows_from(o.mask, f, M);
            o.reward = rows_from(o.reward, f, 1);
            o.done = rows_from(o.done, f, 1);
            o.counter = rows_from(o.counter, f, 1);
            o.ratio = rows_from(o.ratio, f, 1);
            o.ep_ret = rows_from(o.ep_ret, f, 1);
            o.ep_len = rows_from(o.ep_len, f, 1);
        }
        gr[g] = RolloutGroup{&sub[g], &so[(size_t)g * nsets], nullptr, actions + f, rows_from(first_mask, f, M),
                             g == 0 ? stream : (void *)pl->streams[g - 1]};
    }
    hipError_t e = hipEventRecord(pl->fork, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
    for (int g = 1; g < G; ++g) {
        e = hipStreamWaitEvent(pl->streams[g - 1], pl->fork, 0);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");     // nothing is enqueued on a side stream yet
    }
    int rc = rollout_lock_steps(gr, G, nsets, seed, step0, nsteps, draw_first, true, BPP_ROLLOUT_EPS_OF(flags));
    // join, also behind a failed enqueue: whatever did reach a side stream stays ordered in front of the caller's next work
    for (int g = 1; g < G; ++g) {
        e = hipEventRecord(pl->join[g - 1], pl->streams[g - 1]);
        if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)stream, pl->join[g - 1], 0);
        if (e != hipSuccess && rc == 0) rc = hip_fail(e, "hipEventRecord / hipStreamWaitEvent");
    }
    return rc;
}

int bpp_side_create(void **side) {
    const ArgCheck ck{"bpp_side_create"};
    if (!side) return ck.bad("NULL pointer");
    *side = nullptr;
    SideStream *ss = new SideStream();
    if (hipGetDevice(&ss->device) != hipSuccess) {
        (void)side_teardown(ss);
        return ck.bad("no current device");
    }
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    // (a CU mask on this stream -- refills confined to 32 .. 128 CUs so that the others keep all their workgroup slots
    // for the step kernel -- was measured: 0.33 - 0.74 G env steps/s against 1.17 - 1.28 G without, the refill becomes
    // the critical path)
    const char *what = "hipStreamCreateWithPriority";
    hipError_t e = hipStreamCreateWithPriority(&ss->stream, hipStreamNonBlocking, greatest);
    hipEvent_t *ev[3] = {&ss->stepped, &ss->refilled[0], &ss->refilled[1]};
    for (int k = 0; e == hipSuccess && k < 3; ++k) {
        what = "hipEventCreateWithFlags";
        e = hipEventCreateWithFlags(ev[k], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        (void)side_teardown(ss);
        return hip_fail(e, what);
    }
    *side = ss;
    return 0;
}

int bpp_side_destroy(void *side) {
    if (!side) return 0;
    const hipError_t e = side_teardown((SideStream *)side);
    return e == hipSuccess ? 0 : hip_fail(e, "hipStreamDestroy");
}

int bpp_rollout_uniform_stream(const bpp_batch *b, const bpp_step_out *out, int64_t *actions, uint64_t seed, uint64_t step0,
                               int32_t nsteps, const bpp_stream *s, int32_t refill_every, void *side_handle, void *stream) {
    const ArgCheck ck{"bpp_rollout_uniform_stream"};
    if (!b || !s || !out || !out->mask || !actions) return ck.bad("NULL pointer");
    if (nsteps < 0) return ck.bad("negative nsteps");
    const int behind = b->seq_cache ? 4 : 3;   // rows a step launch may touch from the current one on (a cache line refers to the row after next)
    if (b->pool_mode != BPP_POOL_RING || refill_every < 1 || refill_every > s->depth - behind)
        return ck.bad("needs a ring pool and 1 <= refill_every <= depth - 3 (- 4 with seq_cache)");
    int rc = 0;
    // (3 below stands for `behind`.)  With depth >= 2 R + 3 rows per bin the refill that follows a chunk of R lock-steps may run BESIDE the next chunk
    // (it only rewrites rows of finished episodes): it goes to a side stream, and a chunk starts once the refill issued two
    // chunks earlier is complete.  Margin m = rows a bin has from its current episode on when a refill scans it (the
    // previous refill is complete by then: same stream).  A bin advances by at most R episodes per chunk and a step reads
    // two rows ahead, so it needs m >= R + 3 to get through the chunk that runs beside the refill and m + need >= 2 R + 3
    // to get through the one after (this refill complete, the next one running).  The scan guarantees the second
    // (need >= 2 R + 3 - m, `urgent`), which also gives the first for the next scan: m' >= m + need - R >= R + 3.
    SideStream *side = (current_knobs().stream_overlap && s->depth >= 2 * refill_every + behind) ? (SideStream *)side_handle : nullptr;
    hipStream_t main = (hipStream_t)stream;
    if (side) {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev != side->device) return ck.bad("the bpp_side was created on another device");
    }
    const RolloutGroup g{b, nullptr, out, actions, out->mask, stream};
    int32_t chunk = 0;
    for (int32_t done = 0; rc == 0 && done < nsteps; done += refill_every, ++chunk) {
        const int32_t n = nsteps - done < refill_every ? nsteps - done : refill_every;
        if (side && chunk >= 2) (void)hipStreamWaitEvent(main, side->refilled[chunk & 1], 0);
        // only the first chunk draws its first action with a launch of its own: the last step of every chunk but the last draws
        // the next chunk's (the refill in between touches no mask) -- a sampler launch reads the whole mask, 8 / 50 us for 10x10 / 20x20
        rc = rollout_lock_steps(&g, 1, 1, seed, step0 + (uint64_t)done, n, chunk == 0, done + n < nsteps, 0);
        if (rc) break;
        if (!side) {
            rc = bpp_stream_refill(s, stream);
            continue;
        }
        (void)hipEventRecord(side->stepped, main);
        (void)hipStreamWaitEvent(side->stream, side->stepped, 0);
        // beside the lock-steps a short refill matters more than a full ring: a bin gets about twice what the average
        // bin uses in refill_every lock-steps (one sequence per ~9), more only if it would otherwise run out before the
        // refill after the next one is complete
        rc = stream_refill(s, side->stream, refill_every < 7 ? 2 : (refill_every + 5) / 6, 2 * refill_every + behind);
        (void)hipEventRecord(side->refilled[chunk & 1], side->stream);
    }
    if (side) {     // everything enqueued on `stream` after this call sees the refilled ring
        if (chunk >= 2) (void)hipStreamWaitEvent(main, side->refilled[chunk & 1], 0);
        if (chunk >= 1) (void)hipStreamWaitEvent(main, side->refilled[(chunk - 1) & 1], 0);
        const int side_rc = launched(rc == 0 ? "side-stream refill" : nullptr);     // of the unchecked event calls above
        if (rc == 0) rc = side_rc;
        if (rc == 0) rc = bpp_stream_refill(s, stream);     // leave every bin with `depth` rows, as the serial schedule does
    }
    return rc;
}

}  // extern "C"
