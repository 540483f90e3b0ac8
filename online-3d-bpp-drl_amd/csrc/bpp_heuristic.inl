// bpp_heuristic.inl -- the lowest-top packing heuristic (include/bpp_heuristic.h), included by bpp_kernels.hip
// after bpp_placements.inl.  Integer and indexing work: no MFMA, no atomic, one kernel.
//
// A bin belongs to a group of G lanes of one wave: G = 16 (four bins per wave) up to A = 128, the 10x10 form of the rest of the
// library, and the whole wave beyond.  The group's lane g owns the entries m = g, g + G, ... < M in every pass, so neighbouring
// entries -- and therefore the entries of a cluster of ties -- lie on different lanes:
//   stage   the heights of plane 0 -> bytes in LDS, read from memory once
//   rows    rm[m] = max of the fy heights from (i, j) along the row, per half (the two halves differ in fy)
//   keys    K(m) = max of the fx row maxima down the column + z, or INF / INF + 1 (16 bits in LDS); best = the group's minimum
//   ties    the group's count of K(m) = best; with more than one under the smooth rule every tied entry is scored by
//           R(m) - R(h): the edges that touch its window, O(fx fy + perimeter), and the lowest (score, m) wins
// Every lane of a workgroup takes every barrier and every reduction: a group past the last bin works on the last bin's row and
// writes nothing.

namespace {

constexpr int kHeurInf = 0xfffe;     // K of an entry that is on and out of range; off: kHeurInf + 1.  A top is at most 255 + 255.
constexpr int kHeurSmallArea = 128;  // A up to here: 16 lanes per bin

struct HeurArgs {
    const float *obs, *mask;
    int64_t stride;
    int64_t *action;
    int32_t *top;
    int n, W, L, A, M, smooth, bin_lds;
};

// Saturating conversion: clamp, then round to nearest even, then cast.  NaN takes lo (fmaxf returns its other operand).
__device__ __forceinline__ int heur_int(float v, int lo, int hi) { return (int)rintf(fminf(fmaxf(v, (float)lo), (float)hi)); }

template <int G>
__device__ __forceinline__ int heur_group_min(int v) {
    if constexpr (G == 16) return row16_min(v);
    else return wave_min(v);
}
template <int G>
__device__ __forceinline__ int heur_group_sum(int v) {
    if constexpr (G == 16) return row16_isum(v);
    else return wave_sum(v);
}

// What entry m places: the half, the cell (i, j) and the footprint; `fits` = m is in range.
struct HeurEntry {
    int half, pos, i, j, fx, fy;
    bool sides, fits;
};
__device__ __forceinline__ HeurEntry heur_entry(int m, int x, int y, int W, int L, int A) {
    HeurEntry e;
    e.half = m >= A;
    e.pos = m - (e.half ? A : 0);
    e.i = e.pos / L, e.j = e.pos - e.i * L;
    e.fx = e.half ? y : x, e.fy = e.half ? x : y;
    e.sides = e.fx >= 1 && e.fx <= W && e.fy >= 1 && e.fy <= L;
    e.fits = e.sides && e.i + e.fx <= W && e.j + e.fy <= L;
    return e;
}

// R(m) - R(h) of an entry in range: hp is h inside the border at `best`; the window's cells go to `best`.
__device__ __forceinline__ int heur_score(const unsigned char *hb, const HeurEntry &e, int best, int W, int L) {
    const auto hp = [&](int a, int b) { return (a < 0 || a >= W || b < 0 || b >= L) ? best : (int)hb[a * L + b]; };
    int s = 0;
    for (int a = e.i; a < e.i + e.fx; ++a) {
        const int left = hp(a, e.j - 1);
        int cur = hb[a * L + e.j];
        s += abs(best - left) - abs(cur - left);
        for (int b = e.j; b < e.j + e.fy; ++b) {
            const int right = hp(a, b + 1), down = hp(a + 1, b);
            if (b == e.j + e.fy - 1) s += abs(best - right);
            if (a == e.i + e.fx - 1) s += abs(best - down);
            s -= abs(cur - right) + abs(cur - down);
            cur = right;
        }
    }
    for (int b = e.j; b < e.j + e.fy; ++b) {
        const int up = hp(e.i - 1, b);
        s += abs(best - up) - abs((int)hb[e.i * L + b] - up);
    }
    return s;
}

template <int G>
__global__ __launch_bounds__(256) void heuristic_kernel(HeurArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kBins = 256 / G;      // bins of a workgroup
    const int slot = threadIdx.x / G, g = threadIdx.x % G;
    const long long want = (long long)blockIdx.x * kBins + slot;
    const bool live = want < (long long)a.n;
    const size_t bin = live ? (size_t)want : (size_t)a.n - 1;
    const int W = a.W, L = a.L, A = a.A, M = a.M;
    const float *o = a.obs + bin * (size_t)a.stride, *mk = a.mask + bin * (size_t)M;
    unsigned char *hb = smem + (size_t)slot * a.bin_lds;              // [A] heights
    unsigned char *rm = hb + ((A + 3) & ~3);                          // [M] row maxima
    uint16_t *key = (uint16_t *)(rm + ((M + 3) & ~3));                // [M] keys
    const int x = heur_int(o[A], 0, 256), y = heur_int(o[2 * A], 0, 256), z = heur_int(o[3 * A], 0, 255);

    for (int c = g; c < A; c += G) hb[c] = (unsigned char)heur_int(o[c], 0, 255);
    __syncthreads();

    for (int m = g; m < M; m += G) {
        const HeurEntry e = heur_entry(m, x, y, W, L, A);
        if (e.sides && e.j + e.fy <= L) {
            int v = 0;
            for (int b = 0; b < e.fy; ++b) v = max(v, (int)hb[e.pos + b]);
            rm[m] = (unsigned char)v;
        }
    }
    __syncthreads();

    int best = kHeurInf + 1;
    for (int m = g; m < M; m += G) {
        const HeurEntry e = heur_entry(m, x, y, W, L, A);
        int k = kHeurInf + 1;
        if (mk[m] > 0.5f) {
            k = kHeurInf;
            if (e.fits) {
                int v = 0;
                for (int r = 0; r < e.fx; ++r) v = max(v, (int)rm[m + r * L]);
                k = v + z;
            }
        }
        key[m] = (uint16_t)k;       // read back by this lane only
        best = min(best, k);
    }
    best = heur_group_min<G>(best);

    int ties = 0, first = 0x7fffffff;
    for (int m = g; m < M; m += G)
        if (key[m] == best) ++ties, first = min(first, m);
    ties = heur_group_sum<G>(ties);

    int score = 0, pick = first;
    if (a.smooth && best < kHeurInf && ties > 1) {
        score = 0x7fffffff;
        for (int m = g; m < M; m += G) {
            if (key[m] != best) continue;
            const int s = heur_score(hb, heur_entry(m, x, y, W, L, A), best, W, L);
            if (s < score) score = s, pick = m;     // m ascends: the lowest m of a lane's smallest score stays
        }
    }
    const int smallest = heur_group_min<G>(score);
    const int act = heur_group_min<G>(score == smallest ? pick : 0x7fffffff);
    if (live && g == 0) {
        a.action[bin] = (int64_t)act;
        if (a.top) a.top[bin] = best < kHeurInf ? best : -1;
    }
}

struct HeurShape {
    int lanes, bins_per_group, groups, bin_lds;
};

int heur_shape(const ArgCheck &ck, int n, int W, int L, int rotation, HeurShape &s) {
    if (n <= 0) return ck.bad("n must be >= 1");
    if (W < 1 || L < 1) return ck.bad("W and L must be >= 1");
    if (W > kMaxDim || L > kMaxDim || W * L > kMaxArea) return ck.bad("bin too large: need W, L <= 255 and W*L <= 1024");
    if (rotation != 0 && rotation != 1) return ck.bad("rotation must be 0 or 1");
    const int A = W * L, M = A * (1 + rotation);
    s.lanes = A <= kHeurSmallArea ? 16 : kWave;
    s.bins_per_group = 256 / s.lanes;
    s.groups = (int)(((long long)n + s.bins_per_group - 1) / s.bins_per_group);
    s.bin_lds = ((A + 3) & ~3) + ((M + 3) & ~3) + ((2 * M + 3) & ~3);
    return 0;
}

}  // namespace

extern "C" {

int bpp_heuristic_act_info(int32_t W, int32_t L, int32_t rotation, int32_t n, int32_t out[4]) {
    const ArgCheck ck{"bpp_heuristic_act_info"};
    HeurShape s;
    if (const int rc = heur_shape(ck, n, W, L, rotation, s)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = kWave / s.lanes, out[1] = s.bin_lds * s.bins_per_group, out[2] = s.groups, out[3] = s.lanes == kWave;
    return 0;
}

int bpp_heuristic_act(const float *obs, int64_t obs_stride, const float *mask, int32_t n, int32_t W, int32_t L, int32_t rotation,
                      int32_t rule, int64_t *action, int32_t *top, void *stream) {
    const ArgCheck ck{"bpp_heuristic_act"};
    if (!obs || !mask || !action) return ck.bad("NULL pointer");
    HeurShape s;
    if (const int rc = heur_shape(ck, n, W, L, rotation, s)) return rc;
    if (rule != BPP_HEUR_LOWEST_TOP && rule != BPP_HEUR_LOWEST_TOP_PLAIN) return ck.bad("unknown rule");
    if (obs_stride < 4 * (int64_t)(W * L)) return ck.bad("obs_stride < 4 * W * L");
    HeurArgs a;
    a.obs = obs, a.mask = mask, a.stride = obs_stride, a.action = action, a.top = top;
    a.n = n, a.W = W, a.L = L, a.A = W * L, a.M = a.A * (1 + rotation), a.smooth = rule == BPP_HEUR_LOWEST_TOP, a.bin_lds = s.bin_lds;
    const size_t lds = (size_t)s.bin_lds * s.bins_per_group;
    if (s.lanes == 16)
        hipLaunchKernelGGL(heuristic_kernel<16>, dim3(s.groups), dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(heuristic_kernel<kWave>, dim3(s.groups), dim3(256), lds, (hipStream_t)stream, a);
    return launched();
}

}  // extern "C"
