// bpp_placements.inl -- packing plans recorded beside the step (include/bpp_placements.h), included at the end of
// bpp_kernels.hip: the reference's space.boxes / space.flags (envs/bpp0/space.py:23-24,176-177) as a log the step kernel never
// sees.  note (before the step) keeps what the action means for the item on display, commit (after it) turns that into a record
// once the step has said whether the box went in, and reads the height it rests on off the heightmap the step left.
//
// note / commit / clear: one lane per bin, a few bytes each -- an 8-byte note, a 16-byte count record, one 8-byte plan record.
// copy / gather / replay: one wave per bin or plan.  replay keeps a plan's W * L <= 1 024 cells in registers, 1 .. 16 per lane, and
// takes a footprint's maximum with wave_max (bpp_wave.inl): heights are bytes, exact as floats.
//
// The log (opaque to callers): count records uint4 [E] {running count, finished count or -1, finished episode, running episode},
// notes uint2 [E], plan records uint2 [banks][E][capacity], the overflow counter.  A note's byte 3 holds its flags: bit 0 = the
// note is set, bit 1 = which bank holds the bin's running plan (the other one holds the finished plan).

namespace {

constexpr int kPlanLanes = 256;                  // note / commit / clear: lanes per workgroup
constexpr int kPlanWaves = 4;                    // copy / gather / replay: waves per workgroup
constexpr int kReplayCells = kMaxArea / kWave;   // cells of a plan a lane of replay holds
constexpr uint32_t kNoteSet = 1u << 24, kNoteBank = 2u << 24;

struct PlanLog {
    uint4 *meta;
    uint2 *note;
    uint2 *rec;
    int32_t *overflow;
    int32_t E, C, banks;
    __device__ __forceinline__ uint2 *row(int bank, int e) const { return rec + ((size_t)bank * E + e) * (size_t)C; }
    // which bank holds the running plan of a bin whose note word is `flags` (always 0 in a log without finished plans)
    __device__ __forceinline__ int running(uint32_t flags) const { return banks == 2 && (flags & (2u << 24)) ? 1 : 0; }
};

size_t plan_log_bytes(int32_t E, int32_t C, int32_t keep) { return (size_t)E * 24u + (size_t)(keep ? 2 : 1) * E * (size_t)C * 8u + 8u; }

PlanLog plan_log(const void *log, int32_t E, int32_t C, int32_t keep) {
    unsigned char *p = (unsigned char *)const_cast<void *>(log);
    PlanLog g;
    g.E = E, g.C = C, g.banks = keep ? 2 : 1;
    g.meta = (uint4 *)p;
    g.note = (uint2 *)(p + (size_t)E * 16u);
    g.rec = (uint2 *)(p + (size_t)E * 24u);
    g.overflow = (int32_t *)(p + plan_log_bytes(E, C, keep) - 8u);
    return g;
}

// The shape of a log and the log itself, or the refusal of entry point ck.
int check_plan_log(const ArgCheck &ck, const void *log, int32_t E, int32_t C, int32_t keep) {
    if (E < 1 || C < 1 || C > BPP_PLACEMENTS_MAX_CAPACITY) return ck.bad("need E >= 1 and capacity in 1 .. 2^20");
    if (keep != 0 && keep != 1) return ck.bad("keep_finished must be 0 or 1");
    if (!log) return ck.bad("NULL log");
    if (!aligned16(log)) return ck.bad("the log must be 16-byte aligned");
    return 0;
}

__global__ __launch_bounds__(kPlanLanes) void placements_clear_kernel(const PlanLog g) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e == 0) g.overflow[0] = 0, g.overflow[1] = 0;
    if (e >= g.E) return;
    g.meta[e] = make_uint4(0u, 0xffffffffu, 0xffffffffu, 0u);
    g.note[e] = make_uint2(0u, 0u);
}

struct PlanStepArgs {
    PlanLog g;
    const int64_t *ids, *actions;
    const uint8_t *done;
    const bpp_env_state *state;
    const uint8_t *hmap;
    int32_t n, A, rotation;
};

// The bin of launch slot `slot`, or -1 where the slot names none.
__device__ __forceinline__ int plan_slot_bin(const PlanStepArgs &a, int slot) {
    if (!a.ids) return slot;
    const int64_t id = a.ids[slot];
    return (uint64_t)id < (uint64_t)a.g.E ? (int)id : -1;
}

__global__ __launch_bounds__(kPlanLanes) void placements_note_kernel(const PlanStepArgs a) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (slot >= a.n) return;
    const int e = plan_slot_bin(a, slot);
    if (e < 0) return;
    const uint32_t item = a.state[e].item_cur;
    const int64_t act = a.actions[slot];
    const bool flag = a.rotation && act > (int64_t)a.A;       // rotated iff idx > area (strict), as decode_action
    const int64_t idx = flag ? act - a.A : act;
    const uint32_t bank = a.g.note[e].x & kNoteBank;
    uint2 nt = make_uint2(bank, 0u);
    if (act != BPP_ACTION_NOOP && (uint64_t)idx < (uint64_t)a.A) {
        const uint32_t ix = item & 255u, iy = (item >> 8) & 255u, iz = (item >> 16) & 255u;
        nt.x = (flag ? iy : ix) | (flag ? ix : iy) << 8 | iz << 16 | kNoteSet | bank;
        nt.y = (uint32_t)idx | (flag ? 1u << 16 : 0u);
    }
    a.g.note[e] = nt;
}

__global__ __launch_bounds__(kPlanLanes) void placements_commit_kernel(const PlanStepArgs a) {
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (slot >= a.n) return;
    const int e = plan_slot_bin(a, slot);
    if (e < 0) return;
    const uint2 nt = a.g.note[e];
    const bool done = a.done[slot] != 0;
    if (!(nt.x & kNoteSet) && !done) return;       // a bin that was left alone; an action outside the bin ends the episode like any failure
    uint4 m = a.g.meta[e];
    uint32_t bank = nt.x & kNoteBank;
    const uint32_t episode = (uint32_t)a.state[e].episode;
    if (!done) {
        const uint32_t cell = min(nt.y & 0xffffu, (uint32_t)a.A - 1u), z = (nt.x >> 16) & 255u;     // (a note is inside the bin; never read outside it)
        const uint32_t lz = ((uint32_t)a.hmap[(size_t)e * a.A + cell] - z) & 255u;      // the footprint is level at lz + z
        if (m.x < (uint32_t)a.g.C) a.g.row(a.g.running(bank), e)[m.x] = make_uint2((nt.x & 0xffffffu) | lz << 24, nt.y & 0x1ffffu);
        else atomicAdd(a.g.overflow, 1);
        m.x += 1u;
    } else {
        if (a.g.banks == 2) m.y = m.x, m.z = episode - 1u, bank ^= kNoteBank;    // the running plan is the finished one: the banks change roles
        m.x = 0u;
    }
    m.w = episode;
    a.g.meta[e] = m;
    a.g.note[e] = make_uint2(bank, 0u);
}

struct PlanCopyArgs {
    PlanLog g;
    const int64_t *src, *dst;
    int32_t n;
};
__global__ __launch_bounds__(kWave * kPlanWaves) void placements_copy_kernel(const PlanCopyArgs c) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = (int)blockIdx.x * kPlanWaves + (int)(threadIdx.x >> 6);
    if (i >= c.n) return;
    const int64_t s64 = c.src[i], d64 = c.dst[i];
    if ((uint64_t)s64 >= (uint64_t)c.g.E || (uint64_t)d64 >= (uint64_t)c.g.E) return;     // never outside the log
    const int s = (int)s64, d = (int)d64;
    const uint4 m = c.g.meta[s];
    const uint2 nt = c.g.note[s];
    const int run = c.g.running(nt.x);
    for (int b = 0; b < c.g.banks; ++b) {
        const int32_t cnt = (int32_t)(b == run ? m.x : m.y);
        const int nrec = cnt < 0 ? 0 : min(cnt, c.g.C);
        const uint2 *rs = c.g.row(b, s);
        uint2 *rd = c.g.row(b, d);
        for (int k = lane; k < nrec; k += kWave) rd[k] = rs[k];
    }
    if (lane == 0) c.g.meta[d] = m, c.g.note[d] = nt;
}

struct PlanGatherArgs {
    PlanLog g;
    const int64_t *ids;
    uint2 *out;
    int32_t *count, *episode;
    int32_t n, which, stride;
};
__global__ __launch_bounds__(kWave * kPlanWaves) void placements_gather_kernel(const PlanGatherArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = (int)blockIdx.x * kPlanWaves + (int)(threadIdx.x >> 6);
    if (i >= a.n) return;
    const int64_t id = a.ids ? a.ids[i] : (int64_t)i;
    int32_t cnt = -1, ep = -1;
    const uint2 *row = nullptr;
    if ((uint64_t)id < (uint64_t)a.g.E) {
        const int e = (int)id;
        const uint4 m = a.g.meta[e];
        const int run = a.g.running(a.g.note[e].x);
        if (a.which == BPP_PLAN_RUNNING) cnt = (int32_t)m.x, ep = (int32_t)m.w, row = a.g.row(run, e);
        else cnt = (int32_t)m.y, ep = cnt < 0 ? -1 : (int32_t)m.z, row = a.g.row(run ^ 1, e);
    }
    const int nrec = cnt < 0 ? 0 : min(cnt, a.g.C);
    uint2 *out = a.out + (size_t)i * a.stride;
    for (int k = lane; k < a.g.C; k += kWave) out[k] = k < nrec ? row[k] : make_uint2(0u, 0u);
    if (lane == 0) {
        a.count[i] = cnt;
        if (a.episode) a.episode[i] = ep;
    }
}

struct PlanReplayArgs {
    const uint2 *records;
    const int32_t *count;
    uint8_t *hmap;
    int32_t *status, *volume;
    int32_t stride, capacity, n, W, L, H, A, upto;
};
// NC: cells a lane holds, A <= 64 NC (a 10x10 bin needs 2, not 16: the loops below run over what the bin has)
template <int NC>
__global__ __launch_bounds__(kWave * kPlanWaves) void placements_replay_kernel(const PlanReplayArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = (int)blockIdx.x * kPlanWaves + (int)(threadIdx.x >> 6);
    if (i >= a.n) return;                          // a whole wave
    int nb = min(a.count[i], a.capacity);
    if (a.upto >= 0) nb = min(nb, a.upto);
    int h[NC], cx[NC], cy[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {       // cell c = lane + 64 j; a cell past A has cx >= W: under no sound footprint
        const int c = lane + kWave * j;
        cx[j] = c / a.L, cy[j] = c - cx[j] * a.L, h[j] = 0;
    }
    const uint2 *row = a.records + (size_t)i * a.stride;
    int bad = -1, vol = 0;
    for (int k = 0; k < nb; ++k) {                 // every value below is the same in all lanes of the wave
        const uint2 r = row[k];
        const int x = r.x & 255u, y = (r.x >> 8) & 255u, z = (r.x >> 16) & 255u, lz = r.x >> 24, cell = r.y & 0xffffu;
        const int lx = cell / a.L, ly = cell - lx * a.L;
        const bool inside = x >= 1 && y >= 1 && z >= 1 && lx + x <= a.W && ly + y <= a.L;
        float top = 0.0f;
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (cx[j] >= lx && cx[j] < lx + x && cy[j] >= ly && cy[j] < ly + y) top = fmaxf(top, (float)h[j]);
        top = wave_max(top);
        if (!inside || lz != (int)top || lz + z > a.H) {
            bad = k;
            break;
        }
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (cx[j] >= lx && cx[j] < lx + x && cy[j] >= ly && cy[j] < ly + y) h[j] = lz + z;
        vol += x * y * z;
    }
    uint8_t *out = a.hmap + (size_t)i * a.A;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = lane + kWave * j;
        if (c < a.A) out[c] = (uint8_t)h[j];
    }
    if (lane == 0) {
        if (a.status) a.status[i] = bad;
        if (a.volume) a.volume[i] = vol;
    }
}

// What note and commit share: the batch's checks and the launch arguments.
int plan_step_args(const ArgCheck &ck, const bpp_batch *b, const int64_t *ids, int32_t n, const void *log, int32_t capacity,
                   int32_t keep, PlanStepArgs &a) {
    if (!b) return ck.bad("NULL batch");
    if (!b->state || !b->hmap) return ck.bad("NULL pointer in the batch");
    if (b->num_envs < 1 || b->W < 1 || b->L < 1 || b->W > kMaxDim || b->L > kMaxDim || b->W * b->L > kMaxArea)
        return ck.bad("bad geometry in the batch");
    const int rc = check_plan_log(ck, log, b->num_envs, capacity, keep);
    if (rc) return rc;
    if (ids && n < 0) return ck.bad("negative n");
    if ((uintptr_t)ids & 7u) return ck.bad("ids must be 8-byte aligned");
    memset(&a, 0, sizeof a);
    a.g = plan_log(log, b->num_envs, capacity, keep);
    a.ids = ids;
    a.state = b->state;
    a.hmap = b->hmap;
    a.n = ids ? n : b->num_envs;
    a.A = b->W * b->L;
    a.rotation = b->rotation != 0;
    return 0;
}

// cells per lane the replay kernel is compiled for: the power of two that covers A, at most kReplayCells
int replay_cells(int A) {
    int nc = 1;
    while (nc * kWave < A) nc *= 2;
    return nc;
}

unsigned plan_groups(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" {

int64_t bpp_placements_sizes(int32_t E, int32_t capacity, int32_t keep_finished) {
    const ArgCheck ck{"bpp_placements_sizes"};
    if (E < 1 || capacity < 1 || capacity > BPP_PLACEMENTS_MAX_CAPACITY) return ck.bad("need E >= 1 and capacity in 1 .. 2^20");
    if (keep_finished != 0 && keep_finished != 1) return ck.bad("keep_finished must be 0 or 1");
    return (int64_t)plan_log_bytes(E, capacity, keep_finished);
}

int bpp_placements_info(int32_t E, int32_t capacity, int32_t A, int32_t out[6]) {
    const ArgCheck ck{"bpp_placements_info"};
    if (E < 1 || capacity < 1 || capacity > BPP_PLACEMENTS_MAX_CAPACITY || A < 1 || A > kMaxArea)
        return ck.bad("need E >= 1, capacity in 1 .. 2^20 and A in 1 .. 1024");
    if (!out) return ck.bad("NULL out");
    out[0] = kPlanLanes, out[1] = (int32_t)plan_groups(E, kPlanLanes), out[2] = kPlanWaves, out[3] = (int32_t)plan_groups(E, kPlanWaves);
    out[4] = replay_cells(A), out[5] = (int32_t)sizeof(bpp_placement);
    return 0;
}

int bpp_placements_clear(void *log, int32_t E, int32_t capacity, int32_t keep_finished, void *stream) {
    const ArgCheck ck{"bpp_placements_clear"};
    const int rc = check_plan_log(ck, log, E, capacity, keep_finished);
    if (rc) return rc;
    hipLaunchKernelGGL(placements_clear_kernel, dim3(plan_groups(E, kPlanLanes)), dim3(kPlanLanes), 0, (hipStream_t)stream,
                       plan_log(log, E, capacity, keep_finished));
    return launched();
}

int bpp_placements_note(const bpp_batch *b, const int64_t *ids, int32_t n, const int64_t *actions, void *log, int32_t capacity,
                        int32_t keep_finished, void *stream) {
    const ArgCheck ck{"bpp_placements_note"};
    PlanStepArgs a;
    const int rc = plan_step_args(ck, b, ids, n, log, capacity, keep_finished, a);
    if (rc) return rc;
    if (!actions) return ck.bad("NULL actions");
    if ((uintptr_t)actions & 7u) return ck.bad("actions must be 8-byte aligned");
    if (a.n == 0) return 0;
    a.actions = actions;
    hipLaunchKernelGGL(placements_note_kernel, dim3(plan_groups(a.n, kPlanLanes)), dim3(kPlanLanes), 0, (hipStream_t)stream, a);
    return launched();
}

int bpp_placements_commit(const bpp_batch *b, const int64_t *ids, int32_t n, const uint8_t *done, void *log, int32_t capacity,
                          int32_t keep_finished, void *stream) {
    const ArgCheck ck{"bpp_placements_commit"};
    PlanStepArgs a;
    const int rc = plan_step_args(ck, b, ids, n, log, capacity, keep_finished, a);
    if (rc) return rc;
    if (!done) return ck.bad("NULL done");
    if (a.n == 0) return 0;
    a.done = done;
    hipLaunchKernelGGL(placements_commit_kernel, dim3(plan_groups(a.n, kPlanLanes)), dim3(kPlanLanes), 0, (hipStream_t)stream, a);
    return launched();
}

int bpp_placements_copy(void *log, const int64_t *src, const int64_t *dst, int32_t n, int32_t E, int32_t capacity,
                        int32_t keep_finished, void *stream) {
    const ArgCheck ck{"bpp_placements_copy"};
    const int rc = check_plan_log(ck, log, E, capacity, keep_finished);
    if (rc) return rc;
    if (!src || !dst) return ck.bad("NULL pointer");
    if (n < 0) return ck.bad("negative n");
    if (((uintptr_t)src & 7u) || ((uintptr_t)dst & 7u)) return ck.bad("src / dst must be 8-byte aligned");
    if (n == 0) return 0;
    const PlanCopyArgs c{plan_log(log, E, capacity, keep_finished), src, dst, n};
    hipLaunchKernelGGL(placements_copy_kernel, dim3(plan_groups(n, kPlanWaves)), dim3(kWave * kPlanWaves), 0, (hipStream_t)stream, c);
    return launched();
}

int bpp_placements_gather(const void *log, const int64_t *ids, int32_t n, int32_t which, void *out_records, int32_t out_stride,
                          int32_t *out_count, int32_t *out_episode, int32_t E, int32_t capacity, int32_t keep_finished, void *stream) {
    const ArgCheck ck{"bpp_placements_gather"};
    const int rc = check_plan_log(ck, log, E, capacity, keep_finished);
    if (rc) return rc;
    if (which != BPP_PLAN_RUNNING && which != BPP_PLAN_FINISHED) return ck.bad("which must be BPP_PLAN_RUNNING or BPP_PLAN_FINISHED");
    if (which == BPP_PLAN_FINISHED && !keep_finished) return ck.bad("this log keeps no finished plans (keep_finished = 0)");
    if (!out_records || !out_count) return ck.bad("NULL pointer");
    if (ids && n < 0) return ck.bad("negative n");
    if (out_stride < capacity) return ck.bad("out_stride must be >= capacity");
    if (((uintptr_t)ids & 7u) || ((uintptr_t)out_records & 7u) || ((uintptr_t)out_count & 3u) || ((uintptr_t)out_episode & 3u))
        return ck.bad("misaligned buffer");
    const int32_t rows = ids ? n : E;
    if (rows == 0) return 0;
    const PlanGatherArgs a{plan_log(log, E, capacity, keep_finished), ids, (uint2 *)out_records, out_count, out_episode, rows, which, out_stride};
    hipLaunchKernelGGL(placements_gather_kernel, dim3(plan_groups(rows, kPlanWaves)), dim3(kWave * kPlanWaves), 0, (hipStream_t)stream, a);
    return launched();
}

int bpp_placements_replay(const void *records, int32_t stride, int32_t capacity, const int32_t *count, int32_t n, int32_t W,
                          int32_t L, int32_t H, int32_t upto, uint8_t *hmap_out, int32_t *status, int32_t *volume, void *stream) {
    const ArgCheck ck{"bpp_placements_replay"};
    if (!records || !count || !hmap_out) return ck.bad("NULL pointer");
    if (n < 0) return ck.bad("negative n");
    if (capacity < 1 || capacity > BPP_PLACEMENTS_MAX_CAPACITY || stride < capacity) return ck.bad("need capacity in 1 .. 2^20 and stride >= capacity");
    if (W < 1 || L < 1 || H < 1 || W > kMaxArea || L > kMaxArea || H > kMaxDim || W * L > kMaxArea)     // (a plan needs no env: W or L alone may exceed a byte)
        return ck.bad("need W, L >= 1 with W * L <= 1024 and H in 1 .. 255");
    if (((uintptr_t)records & 7u) || ((uintptr_t)count & 3u) || ((uintptr_t)status & 3u) || ((uintptr_t)volume & 3u))
        return ck.bad("misaligned buffer");
    if (n == 0) return 0;
    const PlanReplayArgs a{(const uint2 *)records, count, hmap_out, status, volume, stride, capacity, n, W, L, H, W * L, upto};
    const dim3 grid(plan_groups(n, kPlanWaves)), block(kWave * kPlanWaves);
    const hipStream_t st = (hipStream_t)stream;
    switch (replay_cells(a.A)) {
        case 1: hipLaunchKernelGGL(placements_replay_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(placements_replay_kernel<2>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(placements_replay_kernel<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(placements_replay_kernel<8>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(placements_replay_kernel<kReplayCells>, grid, block, 0, st, a); break;
    }
    return launched();
}

}  // extern "C"
