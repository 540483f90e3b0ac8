// bpp_search_common.inl -- what the three lookahead searches (bpp_reorder.inl, bpp_multibin.inl, bpp_mcts.inl) share,
// included from bpp_kernels.hip right before them.  Every rule of the reference that more than one search restates is
// stated here once: the float32 softmax of a logits row, numpy's argmax tie rules, the 4-plane observation row, the item
// reward; then the host side: the common batch checks and the launch of a one-wave-per-slot kernel (the argument messages,
// ArgCheck, and launched() are the whole library's: bpp_kernels.hip; the wave reductions wave_sum / wave_max / wave_argmax
// are the whole library's too: bpp_wave.inl).
namespace {

constexpr int kSearchWaves = 4;      // waves (= search slots) per workgroup of a one-wave-per-slot kernel

inline dim3 search_grid(int n) { return dim3((unsigned)((n + kSearchWaves - 1) / kSearchWaves)); }   // one wave per slot
inline dim3 search_grid1(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }                         // one thread per item

// First lines of a one-wave-per-slot kernel: the wave's slot i, its lane and its wave number wv in the workgroup.
#define SEARCH_SLOT_PROLOGUE(a)                          \
    const int lane = threadIdx.x & (kWave - 1);          \
    const int wv = (int)(threadIdx.x >> 6);              \
    const int i = (int)blockIdx.x * kSearchWaves + wv;   \
    if (i >= (a).n) return;                              \
    (void)wv;

// A caller's bin id names one of the batch's E bins.
__device__ __forceinline__ bool bin_in_range(int64_t id, int E) { return (uint64_t)id < (uint64_t)E; }

// (bin, scratch bin) of slot i of a search that steps scratch bins; false when either lies outside [0, E).
template <typename Args>
__device__ __forceinline__ bool slot_bins(const Args &a, int i, int &e, int &sid) {
    const int64_t id = a.ids[i], sc = a.scratch[i];
    if (!bin_in_range(id, a.E) || !bin_in_range(sc, a.E)) return false;
    e = (int)id;
    sid = (int)sc;
    return true;
}

// The same, then the slot's bin e and scratch bin sid; ok: both are bins of the batch.
#define SEARCH_SLOT_BINS_PROLOGUE(a) \
    SEARCH_SLOT_PROLOGUE(a)          \
    int e = 0, sid = 0;              \
    const bool ok = slot_bins(a, i, e, sid);

// model_loader.evaluate's softmax of a logits row, float32: mx = max(lg), sum = sum(exp(lg - mx)), lane-strided and then
// the butterfly (bpp_wave.inl).  A probability is expf(lg[c] - mx) / sum (IEEE division).  each(c, expf(lg[c] - mx)) runs in
// the summing pass, for a caller that stores the terms or counts something else along the way.
template <typename Each>
__device__ __forceinline__ void row_softmax_stats(const float *lg, int n, int lane, float &mx, float &sum, Each each) {
    mx = -INFINITY;
    for (int c = lane; c < n; c += kWave) mx = fmaxf(mx, lg[c]);
    mx = wave_max(mx);
    sum = 0.0f;
    for (int c = lane; c < n; c += kWave) {
        const float v = expf(lg[c] - mx);
        each(c, v);
        sum += v;
    }
    sum = wave_sum(sum);
}
__device__ __forceinline__ void row_softmax_stats(const float *lg, int n, int lane, float &mx, float &sum) {
    row_softmax_stats(lg, n, lane, mx, sum, [](int, float) {});
}

// Cells [c0, c0 + 4) of an observation row of n cells per plane (cur_observation: heights h, then the item's x, y, z
// planes): one 16-byte store per plane when n is a multiple of 4 (c0 is one, the row 16-byte aligned), else the cells
// below n one by one.  (multibin_emit_kernel writes the same stores out itself: it came out slower through this function.)
__device__ __forceinline__ void store_obs_quad(float *row, int n, int c0, const float h[4], float fx, float fy, float fz) {
    if ((n & 3) == 0) {
        *(float4 *)(row + c0) = make_float4(h[0], h[1], h[2], h[3]);
        *(float4 *)(row + n + c0) = make_float4(fx, fx, fx, fx);
        *(float4 *)(row + 2 * n + c0) = make_float4(fy, fy, fy, fy);
        *(float4 *)(row + 3 * n + c0) = make_float4(fz, fz, fz, fz);
    } else {
        for (int q = 0; q < 4 && c0 + q < n; ++q) {
            row[c0 + q] = h[q];
            row[n + c0 + q] = fx;
            row[2 * n + c0 + q] = fy;
            row[3 * n + c0 + q] = fz;
        }
    }
}

// bin3D.get_box_ratio() * 10 in float64 of an item x | y << 8 | z << 16.  A volume is at most 255^3 and binvol a positive
// integer, so volume 0 (MCTS: "no reward") gives +0.0 from the same expression and needs no case of its own.
__device__ __forceinline__ uint32_t item_volume(uint32_t it) { return (it & 255u) * ((it >> 8) & 255u) * ((it >> 16) & 255u); }
__device__ __forceinline__ double volume_reward(uint32_t vol, double binvol) { return ((double)vol / binvol) * 10.0; }

// ---- host side --------------------------------------------------------------------------------------------------------
// What every search checks of its batch before anything else (cfg: the search's own struct).  norot: the search's words
// for a batch with rotation.  need_pool: the search reads the batch's static item pool.
int check_search_batch(const bpp_batch *b, const void *cfg, const ArgCheck &ck, const char *norot, bool need_pool) {
    if (!b || !cfg) return ck.bad("NULL pointer");
    const int rc = check_geometry(b->num_envs, b->W, b->L, b->H, b->rotation, b->mask_rule);
    if (rc) return rc;
    if (b->rotation) return ck.bad(norot);
    if (need_pool && b->pool_mode != BPP_POOL_STATIC) return ck.bad("the reorder search needs a static item pool (BPP_POOL_STATIC)");
    if ((need_pool && !b->seq_pool) || !b->hmap || !b->state) return ck.bad("NULL batch buffer");
    return 0;
}

// Launch `kernel` with one wave per slot for n slots / one thread per item for n items; nothing to do for n == 0.
template <typename... KArgs, typename... Args>
int launch_slots(void (*kernel)(KArgs...), int n, void *stream, Args... args) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(kernel, search_grid(n), dim3(kWave * kSearchWaves), 0, (hipStream_t)stream, args...);
    return launched();
}
template <typename... KArgs, typename... Args>
int launch_items(void (*kernel)(KArgs...), int64_t n, void *stream, Args... args) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(kernel, search_grid1(n), dim3(256), 0, (hipStream_t)stream, args...);
    return launched();
}

}  // namespace
