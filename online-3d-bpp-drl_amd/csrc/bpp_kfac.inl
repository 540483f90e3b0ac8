// bpp_kfac.inl -- one Kronecker factor of K-FAC and its running average (include/bpp_kfac.h), included at the end
// of bpp_kernels.hip: X^T X of the rows of acktr/algo/kfac.py:28-63 on the matrix cores, then update_running_stat (:66-70).
//
// The factor is cut into 32 x 32 output tiles, one v_mfma_f32_32x32x2_f32 accumulator each; only tiles on or above the diagonal
// exist.  A workgroup of four waves owns a pair (bi <= bj) of 64-feature blocks -- a wave one tile of the 2 x 2 -- and one
// split of the rows.  It walks its rows a unit at a time: the unit's values for the two feature blocks are staged into LDS in
// the source's own arrangement (for a Conv2d input: the sample's channels with their zero halo), and BOTH operands of the MFMA
// are read from there at `offset of the feature + offset of the row`, two small tables.  An im2col patch is therefore an
// address pattern and is never written anywhere.  The partial tiles go to the workspace; kfac_reduce_kernel adds them per
// element in split order in double, scales, casts, applies the running average and writes both triangles.
//
// The tile -- accumulator, layout, the instruction and its emulated chain -- is bpp_mfma.inl's.  g++ compiles this file too
// (tests/emu); nothing in it differs between the two builds.

namespace {

constexpr int kKfacTile = kMfmaTile;                // side of an output tile
constexpr int kKfacBlock = 2 * kKfacTile;           // features of a block
constexpr int kKfacUnitRows = 64;                   // ROWS: rows staged at a time; NCHW: at most
constexpr int kKfacNchwStride = kKfacUnitRows + 1;  // NCHW: floats between two features of the staged unit (odd: no bank conflicts)
constexpr int kKfacGroups = 1024;                   // workgroups aimed at: pairs x splits
constexpr int kKfacLdsBytes = 64 * 1024;

struct KfacShape {
    int layout, D, nt, nb, pairs, T;          // tiles and blocks per side, block pairs, tiles on or above the diagonal
    long long R, units, ups;                  // rows, units, units per split
    int unit_rows, splits, rows_per_split;
    int B, C, H, W, kh, kw, sh, sw, ph, pw, OH, OW, PH, PW, KK;     // PATCH
    int S, chunks;                            // NCHW: positions per sample, units per sample
    int region, lds;                          // floats of one staged block, bytes of dynamic LDS
};

struct KfacArgs {
    const float *src;
    float *part;
    KfacShape s;
};

// PATCH: the channels [c0, c1) that the features of block bb touch
__host__ __device__ __forceinline__ void kfac_channels(const KfacShape &s, int bb, int &c0, int &c1) {
    const int f0 = bb * kKfacBlock, f1 = min(s.D, f0 + kKfacBlock);
    c0 = f0 / s.KK;
    c1 = (f1 - 1) / s.KK + 1;
}

// where feature f of block bb lies in the staged block (a feature beyond D: anywhere inside, its outputs are never used)
__device__ __forceinline__ int kfac_feature_offset(const KfacShape &s, int bb, int f) {
    if (s.layout == BPP_KFAC_ROWS) return f;
    if (s.layout == BPP_KFAC_NCHW) return f * kKfacNchwStride;
    const int gf = bb * kKfacBlock + f;
    if (gf >= s.D) return 0;
    int c0, c1;
    kfac_channels(s, bb, c0, c1);
    const int c = gf / s.KK, q = gf - c * s.KK, i = q / s.kw;
    return (c - c0) * s.PH * s.PW + i * s.PW + (q - i * s.kw);
}

// what row r of a unit adds to it
__device__ __forceinline__ int kfac_row_offset(const KfacShape &s, int r) {
    if (s.layout == BPP_KFAC_ROWS) return r * kKfacBlock;
    if (s.layout == BPP_KFAC_NCHW) return r;
    const int oy = r / s.OW;
    return oy * s.sh * s.PW + (r - oy * s.OW) * s.sw;
}

// Stage block bb of unit u into img (all 256 lanes); returns the rows of the unit.
__device__ __forceinline__ int kfac_stage(const float *src, const KfacShape &s, long long u, int bb, float *img, int tid) {
    const int f0 = bb * kKfacBlock;
    if (s.layout == BPP_KFAC_ROWS) {
        const long long row0 = u * kKfacUnitRows;
        const int nr = (int)min((long long)kKfacUnitRows, s.R - row0);
        for (int idx = tid; idx < nr * kKfacBlock; idx += 256) {
            const int f = idx & (kKfacBlock - 1), gf = f0 + f;
            img[idx] = gf < s.D ? src[(size_t)(row0 + (idx >> 6)) * (size_t)s.D + (size_t)gf] : 0.0f;
        }
        return nr;
    }
    if (s.layout == BPP_KFAC_NCHW) {
        const long long b = u / s.chunks;
        const int p0 = (int)(u - b * s.chunks) * s.unit_rows, nr = min(s.unit_rows, s.S - p0);
        for (int idx = tid; idx < nr * kKfacBlock; idx += 256) {
            const int f = idx / nr, p = idx - f * nr, gf = f0 + f;
            img[f * kKfacNchwStride + p] = gf < s.D ? src[((size_t)b * (size_t)s.D + (size_t)gf) * (size_t)s.S + (size_t)(p0 + p)] : 0.0f;
        }
        return nr;
    }
    int c0, c1;
    kfac_channels(s, bb, c0, c1);
    const int plane = s.PH * s.PW, n = (c1 - c0) * plane;
    for (int idx = tid; idx < n; idx += 256) {
        const int c = idx / plane, rem = idx - c * plane, y = rem / s.PW, x = rem - y * s.PW;
        const int iy = y - s.ph, ix = x - s.pw;
        const bool in = iy >= 0 && iy < s.H && ix >= 0 && ix < s.W;
        img[idx] = in ? src[(((size_t)u * (size_t)s.C + (size_t)(c0 + c)) * (size_t)s.H + (size_t)iy) * (size_t)s.W + (size_t)ix] : 0.0f;
    }
    return s.OH * s.OW;
}

// acc += A^T-by-B of rows r and r + 1 of the staged unit (row r + 1 counts as zeros when the unit ends at r):
// acc[i][j] = fmaf(x[r + 1][i], x[r + 1][j], fmaf(x[r][i], x[r][j], acc[i][j])).  ta / tb: the feature offsets of the tile's 32
// rows / 32 columns, fa / fb this lane's own (ta[lane & 31], tb[lane & 31]); rtab: the row offsets of the unit.
__device__ __forceinline__ void kfac_mac(MfmaAcc &acc, const float *img, const int *ta, const int *tb, int fa, int fb, const int *rtab,
                                         int r, int nr, int lane) {
    const int k = r + (lane >> 5);                    // the lane's own operands, the only ones the device fetches
    const bool ok = k < nr;
    const int ro = rtab[ok ? k : r];
    const float a = ok ? img[fa + ro] : 0.0f, b = ok ? img[fb + ro] : 0.0f;
    const auto x = [&](const int *t, int f, int kk) { return r + kk < nr ? img[t[f] + rtab[r + kk]] : 0.0f; };
    mfma_step(acc, lane, a, b, [&](int i, int kk) { return x(ta, i, kk); }, [&](int kk, int j) { return x(tb, j, kk); });
}

// index of tile (ti <= tj) among the tiles on or above the diagonal, row by row
__host__ __device__ __forceinline__ int kfac_tile_index(int nt, int ti, int tj) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

// grid = pairs x splits
__global__ __launch_bounds__(256) void kfac_partial_kernel(KfacArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const KfacShape &s = a.s;
    float *img = (float *)smem;
    int *ftab = (int *)(img + (s.nb > 1 ? 2 : 1) * s.region);     // [2][64]: feature offsets of block bi, of block bj
    int *rtab = ftab + 2 * kKfacBlock;                            // [unit_rows]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int pair = (int)(blockIdx.x / (unsigned)s.splits), split = (int)(blockIdx.x % (unsigned)s.splits);
    int bi = 0, rest = pair;
    while (rest >= s.nb - bi) {
        rest -= s.nb - bi;
        ++bi;
    }
    const int bj = bi + rest;
    float *img_j = bj != bi ? img + s.region : img;
    if (tid < 2 * kKfacBlock) {
        const int second = tid >> 6;
        ftab[tid] = (second && bj != bi ? s.region : 0) + kfac_feature_offset(s, second ? bj : bi, tid & (kKfacBlock - 1));
    }
    for (int r = tid; r < s.unit_rows; r += 256) rtab[r] = kfac_row_offset(s, r);
    __syncthreads();
    const int wi = wave >> 1, wj = wave & 1;
    const int ti = 2 * bi + wi, tj = 2 * bj + wj;
    const bool active = ti < s.nt && tj < s.nt && tj >= ti;
    const int *ta = ftab + wi * kKfacTile, *tb = ftab + kKfacBlock + wj * kKfacTile;
    const int fa = ta[lane & 31], fb = tb[lane & 31];
    MfmaAcc acc;
#pragma unroll
    for (int k = 0; k < kMfmaSlots; ++k) acc[k] = 0.0f;
    const long long u0 = (long long)split * s.ups, u1 = min(s.units, u0 + s.ups);
    for (long long u = u0; u < u1; ++u) {
        const int nr = kfac_stage(a.src, s, u, bi, img, tid);
        if (bj != bi) kfac_stage(a.src, s, u, bj, img_j, tid);
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int r = 0; r < nr; r += 2) kfac_mac(acc, img, ta, tb, fa, fb, rtab, r, nr, lane);
        }
        __syncthreads();
    }
    if (active) {
        float *out = a.part + ((size_t)split * (size_t)s.T + (size_t)kfac_tile_index(s.nt, ti, tj)) * 1024u;
#pragma unroll
        for (int k = 0; k < kMfmaSlots; ++k) out[k * kWave + lane] = acc[k];
    }
}

// One lane per element of a tile on or above the diagonal: the partials of the splits in order, in double -> aa -> m.
__global__ __launch_bounds__(256) void kfac_reduce_kernel(const float *part, float *m, int D, int nt, int T, int splits, double scale,
                                                          float c1, float c2, int first) {
    const long long e = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (e >= (long long)T * 1024) return;
    const int tile = (int)(e >> 10), q = (int)(e & 1023), slot = q >> 6, lane = q & 63;
    int ti = 0, rest = tile;
    while (rest >= nt - ti) {
        rest -= nt - ti;
        ++ti;
    }
    const int tj = ti + rest;
    const int row = mfma_slot_row(slot, lane), col = lane & 31;
    const int i = ti * kKfacTile + row, j = tj * kKfacTile + col;
    if (i >= D || j >= D || j < i) return;
    double sum = 0.0;
    for (int sp = 0; sp < splits; ++sp) sum = sum + (double)part[((size_t)sp * (size_t)T + (size_t)tile) * 1024u + (size_t)q];
    const float aa = (float)(sum * scale);
    float v = first ? aa : m[(size_t)i * (size_t)D + (size_t)j];
    v = ((v * c1) + aa) * c2;
    m[(size_t)i * (size_t)D + (size_t)j] = v;
    m[(size_t)j * (size_t)D + (size_t)i] = v;
}

int kfac_shape(int32_t layout, const int32_t *g, const ArgCheck &ck, KfacShape &s) {
    if (!g) return ck.bad("NULL geom");
    memset(&s, 0, sizeof s);
    s.layout = layout;
    long long D, R;
    if (layout == BPP_KFAC_PATCH) {
        s.B = g[0], s.C = g[1], s.H = g[2], s.W = g[3], s.kh = g[4], s.kw = g[5], s.sh = g[6], s.sw = g[7], s.ph = g[8], s.pw = g[9];
        if (s.B < 1 || s.C < 1 || s.H < 1 || s.W < 1 || s.kh < 1 || s.kw < 1) return ck.bad("every extent must be >= 1");
        if (s.sh < 1 || s.sw < 1) return ck.bad("stride must be >= 1");
        if (s.ph < 0 || s.pw < 0) return ck.bad("padding must be >= 0");
        if ((double)s.H + 2.0 * s.ph > 32768.0 || (double)s.W + 2.0 * s.pw > 32768.0 || (double)s.C * s.kh * s.kw > 2147483647.0)
            return ck.bad("image too large");
        s.PH = s.H + 2 * s.ph, s.PW = s.W + 2 * s.pw;
        if (s.kh > s.PH || s.kw > s.PW) return ck.bad("kernel larger than the padded image");
        s.OH = (s.PH - s.kh) / s.sh + 1, s.OW = (s.PW - s.kw) / s.sw + 1;
        s.KK = s.kh * s.kw;
        D = (long long)s.C * s.KK;
        if ((double)s.B * s.OH * s.OW > 2147483647.0 || (double)s.B * s.C * s.H * s.W > 4.0e18) return ck.bad("too many rows");
        R = (long long)s.B * s.OH * s.OW;
        s.units = s.B, s.unit_rows = s.OH * s.OW;
    } else if (layout == BPP_KFAC_ROWS) {
        R = g[0], D = g[1];
        if (R < 1 || D < 1) return ck.bad("R and D must be >= 1");
        s.units = (R + kKfacUnitRows - 1) / kKfacUnitRows, s.unit_rows = kKfacUnitRows;
        s.region = kKfacUnitRows * kKfacBlock;
    } else if (layout == BPP_KFAC_NCHW) {
        s.B = g[0], D = g[1], s.S = g[2];
        if (s.B < 1 || D < 1 || s.S < 1) return ck.bad("every extent must be >= 1");
        if ((double)s.B * s.S > 2147483647.0) return ck.bad("too many rows");
        R = (long long)s.B * s.S;
        s.chunks = (s.S + kKfacUnitRows - 1) / kKfacUnitRows;
        s.units = (long long)s.B * s.chunks, s.unit_rows = (s.S + s.chunks - 1) / s.chunks;      // equal chunks of <= 64 positions
        s.region = kKfacBlock * kKfacNchwStride;
    } else {
        return ck.bad("unknown layout");
    }
    s.D = (int)D, s.R = R;
    s.nt = (s.D + kKfacTile - 1) / kKfacTile, s.nb = (s.D + kKfacBlock - 1) / kKfacBlock;
    if (s.nb > 1024) return ck.bad("D too large");
    s.pairs = s.nb * (s.nb + 1) / 2, s.T = s.nt * (s.nt + 1) / 2;
    if (layout == BPP_KFAC_PATCH) {
        int most = 0;
        for (int bb = 0; bb < s.nb; ++bb) {
            int c0, c1;
            kfac_channels(s, bb, c0, c1);
            most = max(most, c1 - c0);
        }
        if ((double)most * s.PH * s.PW > (double)kKfacLdsBytes) return ck.bad("the staged channels of a sample do not fit the LDS");
        s.region = most * s.PH * s.PW;
    }
    const long long lds = ((long long)(s.nb > 1 ? 2 : 1) * s.region + 2 * kKfacBlock + s.unit_rows) * 4;
    if (lds > kKfacLdsBytes) return ck.bad("the staged channels of a sample do not fit the LDS");
    s.lds = (int)lds;
    const long long most_splits = max(1, kKfacGroups / s.pairs);
    s.ups = (s.units + most_splits - 1) / most_splits;
    s.splits = (int)((s.units + s.ups - 1) / s.ups);
    long long rps;
    if (layout == BPP_KFAC_NCHW) rps = (s.ups / s.chunks) * s.S + min((s.ups % s.chunks) * s.unit_rows, (long long)s.S);
    else rps = s.ups * s.unit_rows;
    s.rows_per_split = (int)min(rps, 2147483647LL);
    return 0;
}

}  // namespace

extern "C" {

size_t bpp_kfac_factor_workspace(int32_t layout, const int32_t geom[]) {
    KfacShape s;
    if (kfac_shape(layout, geom, ArgCheck{"bpp_kfac_factor_workspace"}, s)) return 0;
    return (size_t)s.splits * (size_t)s.T * 1024u * sizeof(float);
}

int bpp_kfac_factor_info(int32_t layout, const int32_t geom[], int32_t out[6]) {
    const ArgCheck ck{"bpp_kfac_factor_info"};
    KfacShape s;
    if (const int rc = kfac_shape(layout, geom, ck, s)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = s.D, out[1] = (int32_t)s.R, out[2] = kKfacTile, out[3] = s.rows_per_split, out[4] = s.splits, out[5] = (int32_t)min((long long)s.rows_per_split, s.R);
    return 0;
}

int bpp_kfac_factor(const float *src, int32_t layout, const int32_t geom[], float *m, double scale, double stat_decay, int32_t first,
                    void *workspace, void *stream) {
    const ArgCheck ck{"bpp_kfac_factor"};
    if (!src || !geom || !m || !workspace) return ck.bad("NULL pointer");
    KfacArgs a;
    if (const int rc = kfac_shape(layout, geom, ck, a.s)) return rc;
    if (!(stat_decay > 0.0 && stat_decay < 1.0)) return ck.bad("stat_decay must lie in (0, 1)");
    a.src = src, a.part = (float *)workspace;
    const KfacShape &s = a.s;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kfac_partial_kernel, dim3((unsigned)(s.pairs * s.splits)), dim3(256), (size_t)s.lds, st, a);
    if (const int rc = launched()) return rc;
    const long long lanes = (long long)s.T * 1024;
    hipLaunchKernelGGL(kfac_reduce_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, (const float *)workspace, m, s.D, s.nt,
                       s.T, s.splits, scale, (float)(stat_decay / (1.0 - stat_decay)), (float)(1.0 - stat_decay), (int)(first != 0));
    return launched();
}

}  // extern "C"
