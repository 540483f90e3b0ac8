// bpp_policy_heads_train.inl -- the training pass of the six Linear layers of CNNPro's heads (include/bpp_policy_heads_train.h;
// DESIGN.md 3.18), included at the end of bpp_kernels.hip after bpp_policy_train.inl: the forward that keeps its hidden vectors,
// the gradient at the head features and at every pre-activation, and the gradient of every Linear weight and bias, float32 on
// the matrix cores.
//
// Forward: policy_head_kernel<true> (bpp_policy.inl), the inference kernel with one more store.
//
// policy_heads_grad_kernel: its sibling on the second blob.  A workgroup owns 64 bins and one head, the same LDS.  go' passes
// through the chunk 64 output features at a time (masked by pred > 0 for the mask head, and written to grad_out_mask), Dh = go' x W2
// lands where the forward kept its hidden vector; one pass over it reads `hidden`, applies the mask and writes Gh to the LDS and
// to grad_hidden in rows; grad_feat = Gh x W1 goes from the accumulators to memory, 32 consecutive floats of a row per half wave.
// A chunk of odd length gets a row of zeros behind it, so that policy_chain sees an even K; the weight that row meets is the
// float behind W2, which the blob's order (W2 in front of its head's W1) keeps inside the blob.
//
// policy_heads_wgrad_kernel: policy_wgrad_kernel's sibling for plain rows.  A workgroup of four waves owns a block of 64 rows k by
// 128 columns of one matrix [K + 1][OC] (a wave one row tile and two column tiles) and one split of the bins.  It stages 32 bins
// at a time: their input rows (the slice of feat, or hidden) with a column of ones at feature K, and their G rows.  The MFMA's A
// operand is read transposed from the former -- lane l takes feature l & 31 of bin r + (l >> 5) -- the B operand from the latter.
// The partial tiles go to the workspace; policy_heads_wgrad_reduce_kernel adds them per element in split order in double and
// casts once.  Both staged arrays have a row stride of 32 mod 64 floats: the two bins a wave reads at once lie in different
// halves of the banks.
//
// The tile -- accumulator, layout, the instruction and its emulated chain -- is bpp_mfma.inl's; the chain is bpp_policy.inl's.
// g++ compiles this file too (tests/emu); nothing in it differs between the two builds.

namespace {

constexpr int kPhMatrices = 6;                    // actor.3, dist.linear, mask.3, mask.5, critic.3, critic_linear: the blob's order
constexpr int kPhSplitBins = 128;                 // bins of a split
constexpr int kPhBlockRows = 2 * kPolTile;        // rows k of a weight-gradient workgroup
constexpr int kPhBlockCols = 4 * kPolTile;        // its columns
constexpr int kPhStage = 32;                      // bins staged at a time
constexpr int kPhXStride = kPhBlockRows + 32;     // floats between two staged input rows
constexpr int kPhGStride = kPhBlockCols + 32;     // floats between two staged G rows
constexpr int kPhWgLds = kPhStage * (kPhXStride + kPhGStride) * 4;
constexpr int kPhPartial = 8 * 1024;              // floats a workgroup leaves in the workspace: 4 waves x 2 tiles

struct PhShape {
    PolShape p;
    int splits, blocks;
    int rows[kPhMatrices], cols[kPhMatrices], cb[kPhMatrices];      // K + 1, OC, column blocks
    int blk0[kPhMatrices + 1];                    // first block of a matrix
    long long goff[kPhMatrices + 1];              // where a matrix starts in grad_weights
    long long wb2[3], wb1[3], wb_total;           // offsets into weights_bwd of a head's W2 [Mh][H] and W1 [H][K1]
};

struct PhGradArgs {
    const float *hidden, *pred, *go[3], *wb;      // go: grad_logits, grad_pred, grad_value (NULL: the head contributes nothing)
    float *grad_feat, *grad_hidden, *grad_out_mask;
    PhShape s;
};

struct PhWgradArgs {
    const float *x[kPhMatrices], *g[kPhMatrices]; // input rows and G rows of a matrix (g NULL: the head contributes nothing)
    int xstride[kPhMatrices];
    float *part;
    PhShape s;
};

struct PhReduceArgs {
    const float *part;
    float *gw;
    int live[3];
    PhShape s;
};

// grid = ceil(n / 64) * 3: workgroup g takes bin tile g / 3 and head g % 3
__global__ __launch_bounds__(256) void policy_heads_grad_kernel(PhGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PolShape &s = a.s.p;
    float *hid = (float *)smem;                       // [H][65]: Dh, then Gh, of hidden feature h of bin b at h * 65 + b
    float *chunk = hid + s.H * kPolStride;            // [64][65]: the staged go', the same way
    int *itab = (int *)(chunk + kPolChunk * kPolStride);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31;
    const int head = (int)(blockIdx.x % 3u);
    const int K1 = (head == 2 ? 4 : 8) * s.A, f0 = head * 8 * s.A, Mh = head == 2 ? 1 : s.M, F = kPolHeadC * s.A;
    const long long bin0 = (long long)(blockIdx.x / 3u) * kPolT;
    const int nb = (int)min((long long)kPolT, (long long)s.n - bin0);
    float *ghid = a.grad_hidden + ((size_t)head * (size_t)s.n + (size_t)bin0) * (size_t)s.H;
    const float *go = a.go[head];
    if (!go) {
        for (int idx = tid; idx < nb * K1; idx += 256) {
            const int b = idx / K1;
            a.grad_feat[(size_t)(bin0 + b) * (size_t)F + (size_t)(f0 + idx - b * K1)] = 0.0f;
        }
        for (int idx = tid; idx < nb * s.H; idx += 256) ghid[idx] = 0.0f;
        if (head == 1)
            for (int idx = tid; idx < nb * Mh; idx += 256) a.grad_out_mask[(size_t)bin0 * (size_t)Mh + (size_t)idx] = 0.0f;
        return;
    }
    const float *w2 = a.wb + a.s.wb2[head], *w1 = a.wb + a.s.wb1[head];
    if (tid < kPolT) itab[tid] = tid;
    const int rtile = wave & 1, cgroup = wave >> 1;
    const int *rt = itab + rtile * kPolTile;
    const int ro = rtile * kPolTile + col;
    // Dh = go' x W2: a pass covers 256 hidden features, a wave 32 bins by 128 of them
    for (int h0 = 0; h0 < s.H; h0 += 8 * kPolTile) {
        const int col0 = h0 + cgroup * 4 * kPolTile;
        MfmaAcc acc[4];
        mfma_fill(acc, [](int) { return 0.0f; });
        for (int m0 = 0; m0 < Mh; m0 += kPolChunk) {
            const int kc = min(kPolChunk, Mh - m0), kp = (kc + 1) & ~1;       // kp: kc made even by a row of zeros
            for (int idx = tid; idx < kPolT * kp; idx += 256) {
                const int b = idx / kp, kk = idx - b * kp;
                float g = 0.0f;
                if (kk < kc && b < nb) {
                    const size_t at = (size_t)(bin0 + b) * (size_t)Mh + (size_t)(m0 + kk);
                    g = go[at];
                    if (head == 1) {
                        g = a.pred[at] > 0.0f ? g : 0.0f;
                        if (h0 == 0) a.grad_out_mask[at] = g;
                    }
                }
                chunk[kk * kPolStride + b] = g;
            }
            __syncthreads();
            if (col0 < s.H) policy_chain<4, 8>(acc, chunk, rt, ro, nullptr, kPolStride, kp, w2 + (size_t)m0 * (size_t)s.H, s.H, col0, s.H, lane);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = col0 + kPolTile * t + col;
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q)
                if (c < s.H) hid[c * kPolStride + rtile * kPolTile + mfma_slot_row(q, lane)] = acc[t][q];
        }
    }
    __syncthreads();
    // Gh = hidden > 0 ? Dh : 0, in place and to grad_hidden
    const float *hrow = a.hidden + ((size_t)head * (size_t)s.n + (size_t)bin0) * (size_t)s.H;
    for (int idx = tid; idx < kPolT * s.H; idx += 256) {
        const int b = idx / s.H;
        float *d = hid + (idx - b * s.H) * kPolStride + b;
        float g = 0.0f;
        if (b < nb) {
            g = hrow[idx] > 0.0f ? *d : 0.0f;
            ghid[idx] = g;
        }
        *d = g;
    }
    __syncthreads();
    // grad_feat = Gh x W1: a wave takes 32 bins by 128 input features at a time
    for (int col0 = cgroup * 4 * kPolTile; col0 < K1; col0 += 8 * kPolTile) {
        MfmaAcc acc[4];
        mfma_fill(acc, [](int) { return 0.0f; });
        policy_chain<4, 8>(acc, hid, rt, ro, nullptr, kPolStride, s.H, w1, K1, col0, K1, lane);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = col0 + kPolTile * t + col;
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q) {
                const int b = rtile * kPolTile + mfma_slot_row(q, lane);
                if (c < K1 && b < nb) a.grad_feat[(size_t)(bin0 + b) * (size_t)F + (size_t)(f0 + c)] = acc[t][q];
            }
        }
    }
}

// grid = blocks x splits: workgroup g takes block g % blocks and split g / blocks
__global__ __launch_bounds__(256) void policy_heads_wgrad_kernel(PhWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PhShape &s = a.s;
    float *xs = (float *)smem;                            // [32][kPhXStride]: input feature f0 + i of staged bin r at r * stride + i
    float *gs = xs + kPhStage * kPhXStride;               // [32][kPhGStride]: G column c0 + j of staged bin r
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int blk = (int)(blockIdx.x % (unsigned)s.blocks), split = (int)(blockIdx.x / (unsigned)s.blocks);
    int m = 0;
    while (blk >= s.blk0[m + 1]) ++m;
    const float *g = a.g[m];
    if (!g) return;                                       // the reduce kernel writes this head's zeros
    const int K = s.rows[m] - 1, OC = s.cols[m], local = blk - s.blk0[m];
    const int f0 = (local / s.cb[m]) * kPhBlockRows, c0 = (local % s.cb[m]) * kPhBlockCols;
    const int wi = wave >> 1, wj = wave & 1;
    // a wave with no row below K + 1 or no column below OC does nothing and writes nothing; inside an active wave the rows from
    // K + 1 and the columns from OC on are staged as zeros and the reduce kernel never reads them
    const bool active = f0 + wi * kPolTile <= K && c0 + wj * 2 * kPolTile < OC;
    const float *xa = xs + wi * kPolTile, *ga = gs + wj * 2 * kPolTile;
    MfmaAcc acc[2];
    mfma_fill(acc, [](int) { return 0.0f; });
    const float *x = a.x[m];
    const size_t xstride = (size_t)a.xstride[m];
    const long long b0 = (long long)split * kPhSplitBins, b1 = min((long long)s.p.n, b0 + kPhSplitBins);
    for (long long bs = b0; bs < b1; bs += kPhStage) {
        const int cnt = (int)min((long long)kPhStage, b1 - bs);
        for (int idx = tid; idx < kPhStage * kPhBlockRows; idx += 256) {
            const int r = idx / kPhBlockRows, i = idx - r * kPhBlockRows, k = f0 + i;
            xs[r * kPhXStride + i] = r < cnt ? (k < K ? x[(size_t)(bs + r) * xstride + (size_t)k] : k == K ? 1.0f : 0.0f) : 0.0f;
        }
        for (int idx = tid; idx < kPhStage * kPhBlockCols; idx += 256) {
            const int r = idx / kPhBlockCols, j = idx - r * kPhBlockCols, c = c0 + j;
            gs[r * kPhGStride + j] = r < cnt && c < OC ? g[(size_t)(bs + r) * (size_t)OC + (size_t)c] : 0.0f;
        }
        __syncthreads();
        if (active) {
            // two bins per instruction; the bin behind an odd count is a staged row of zeros: fmaf(0, 0, acc)
            for (int r = 0; r < cnt; r += 2) {
                const float xv = xa[(r + half) * kPhXStride + col];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    mfma_step(acc[t], lane, xv, ga[(r + half) * kPhGStride + kPolTile * t + col],
                              [&](int i, int q) { return xa[(r + q) * kPhXStride + i]; },
                              [&](int q, int j) { return ga[(r + q) * kPhGStride + kPolTile * t + j]; });
            }
        }
        __syncthreads();
    }
    if (active) {
        float *out = a.part + (((size_t)split * (size_t)s.blocks + (size_t)blk) * 4u + (size_t)wave) * 2048u;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q) out[t * 1024 + q * kWave + lane] = acc[t][q];
        }
    }
}

// One lane per float of grad_weights: the partials of the splits in order, in double, cast once; zero for a head without gradient.
__global__ __launch_bounds__(256) void policy_heads_wgrad_reduce_kernel(PhReduceArgs a) {
    const PhShape &s = a.s;
    const long long e = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (e >= s.goff[kPhMatrices]) return;
    int m = 0;
    while (e >= s.goff[m + 1]) ++m;
    if (!a.live[m >> 1]) {
        a.gw[e] = 0.0f;
        return;
    }
    const int OC = s.cols[m], idx = (int)(e - s.goff[m]);
    const int k = idx / OC, oc = idx - k * OC;
    const int blk = s.blk0[m] + (k / kPhBlockRows) * s.cb[m] + oc / kPhBlockCols;
    const int wave = 2 * ((k % kPhBlockRows) / kPolTile) + (oc % kPhBlockCols) / (2 * kPolTile), t = (oc % (2 * kPolTile)) / kPolTile;
    const size_t stride = (size_t)s.blocks * kPhPartial;
    const float *at = a.part + (((size_t)blk * 4u + (size_t)wave) * 2u + (size_t)t) * 1024u + (size_t)mfma_stored_at(k % kPolTile, oc % kPolTile);
    double sum = 0.0;
    for (int sp = 0; sp < s.splits; ++sp) sum = sum + (double)at[(size_t)sp * stride];
    a.gw[e] = (float)sum;
}

int policy_heads_shape(const int32_t *g, int32_t n, bool need_n, const ArgCheck &ck, PhShape &s) {
    if (const int rc = policy_shape(g, n, need_n, ck, s.p, 1)) return rc;
    const PolShape &p = s.p;
    long long at = 0, wb = 0;
    s.blk0[0] = 0;
    for (int h = 0; h < 3; ++h) {
        const int K1 = (h == 2 ? 4 : 8) * p.A, Mh = h == 2 ? 1 : p.M;
        s.rows[2 * h] = K1 + 1, s.cols[2 * h] = p.H, s.rows[2 * h + 1] = p.H + 1, s.cols[2 * h + 1] = Mh;
        s.wb2[h] = wb, wb += (long long)Mh * p.H;
        s.wb1[h] = wb, wb += (long long)p.H * K1;
    }
    s.wb_total = wb;
    for (int m = 0; m < kPhMatrices; ++m) {
        s.goff[m] = at;
        at += (long long)s.rows[m] * s.cols[m];
        s.cb[m] = (s.cols[m] + kPhBlockCols - 1) / kPhBlockCols;
        s.blk0[m + 1] = s.blk0[m] + ((s.rows[m] + kPhBlockRows - 1) / kPhBlockRows) * s.cb[m];
    }
    s.goff[kPhMatrices] = at;
    s.blocks = s.blk0[kPhMatrices];
    const long long splits = need_n ? ((long long)n + kPhSplitBins - 1) / kPhSplitBins : 0;
    if (splits * s.blocks > 2147483647LL) return ck.bad("n too large");
    s.splits = (int)splits;
    return 0;
}

size_t policy_heads_workspace(const PhShape &s) { return (size_t)s.splits * (size_t)s.blocks * kPhPartial * sizeof(float); }

}  // namespace

extern "C" {

size_t bpp_policy_heads_backward_workspace(const int32_t geom[], int32_t n) {
    PhShape s;
    if (policy_heads_shape(geom, n, true, ArgCheck{"bpp_policy_heads_backward_workspace"}, s)) return 0;
    return policy_heads_workspace(s);
}

size_t bpp_policy_heads_backward_weights_floats(const int32_t geom[]) {
    PhShape s;
    if (policy_heads_shape(geom, 0, false, ArgCheck{"bpp_policy_heads_backward_weights_floats"}, s)) return 0;
    return (size_t)s.wb_total;
}

int bpp_policy_heads_backward_info(const int32_t geom[], int32_t n, int32_t out[8]) {
    const ArgCheck ck{"bpp_policy_heads_backward_info"};
    PhShape s;
    if (out) out[6] = 0;
    if (const int rc = policy_heads_shape(geom, n, true, ck, s)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = kPolT, out[1] = s.p.head_lds, out[2] = kPhSplitBins, out[3] = s.splits, out[4] = min(kPhSplitBins, n), out[5] = kPhWgLds;
    out[6] = 1, out[7] = s.blocks;
    return 0;
}

int bpp_policy_heads_forward_train(const float *feat, int32_t n, const int32_t geom[], const float *weights, float *value, float *logits,
                                   float *pred, float *hidden, void *stream) {
    const ArgCheck ck{"bpp_policy_heads_forward_train"};
    if (!feat || !geom || !weights || !value || !logits || !pred || !hidden) return ck.bad("NULL pointer");
    PolHeadArgs h;
    if (const int rc = policy_shape(geom, n, true, ck, h.s, 1)) return rc;
    h.feat = feat, h.w = weights, h.hidden = hidden, h.nheads = 3;
    h.out[0] = logits, h.out[1] = pred, h.out[2] = value;
    for (int k = 0; k < 3; ++k) h.heads[k] = k;
    return launch_large_lds<policy_head_kernel<true>>(dim3((unsigned)(((long long)n + kPolT - 1) / kPolT) * 3u), dim3(256), h.s.head_lds,
                                                      kPolLdsBytes, (hipStream_t)stream, h);
}

int bpp_policy_heads_backward(const float *feat, const float *hidden, const float *pred, const float *grad_value, const float *grad_logits,
                              const float *grad_pred, int32_t n, const int32_t geom[], const float *weights_bwd, float *grad_feat,
                              float *grad_hidden, float *grad_out_mask, float *grad_weights, void *workspace, size_t workspace_bytes,
                              void *stream) {
    const ArgCheck ck{"bpp_policy_heads_backward"};
    if (!feat || !hidden || !pred || !geom || !weights_bwd || !grad_feat || !grad_hidden || !grad_out_mask || !grad_weights || !workspace)
        return ck.bad("NULL pointer");
    if (!grad_value && !grad_logits && !grad_pred) return ck.bad("at least one of grad_value, grad_logits and grad_pred must be given");
    PhGradArgs g;
    if (const int rc = policy_heads_shape(geom, n, true, ck, g.s)) return rc;
    const PhShape &s = g.s;
    if (workspace_bytes < policy_heads_workspace(s)) return ck.bad("workspace smaller than bpp_policy_heads_backward_workspace");
    const hipStream_t st = (hipStream_t)stream;
    const size_t nH = (size_t)n * (size_t)s.p.H;
    g.hidden = hidden, g.pred = pred, g.wb = weights_bwd;
    g.go[0] = grad_logits, g.go[1] = grad_pred, g.go[2] = grad_value;
    g.grad_feat = grad_feat, g.grad_hidden = grad_hidden, g.grad_out_mask = grad_out_mask;
    if (const int rc = launch_large_lds<policy_heads_grad_kernel>(dim3((unsigned)(((long long)n + kPolT - 1) / kPolT) * 3u), dim3(256), s.p.head_lds,
                                                                  kPolLdsBytes, st, g))
        return rc;
    PhWgradArgs w;
    const float *rows[3] = {grad_logits, grad_pred ? grad_out_mask : nullptr, grad_value};     // the G rows of a head's second Linear
    for (int h = 0; h < 3; ++h) {
        w.x[2 * h] = feat + (size_t)h * 8u * (size_t)s.p.A, w.xstride[2 * h] = kPolHeadC * s.p.A;
        w.g[2 * h] = rows[h] ? grad_hidden + (size_t)h * nH : nullptr;
        w.x[2 * h + 1] = hidden + (size_t)h * nH, w.xstride[2 * h + 1] = s.p.H;
        w.g[2 * h + 1] = rows[h];
    }
    w.part = (float *)workspace, w.s = s;
    hipLaunchKernelGGL(policy_heads_wgrad_kernel, dim3((unsigned)s.blocks * (unsigned)s.splits), dim3(256), kPhWgLds, st, w);
    if (const int rc = launched()) return rc;
    PhReduceArgs r;
    r.part = (const float *)workspace, r.gw = grad_weights, r.s = s;
    for (int h = 0; h < 3; ++h) r.live[h] = rows[h] != nullptr;
    hipLaunchKernelGGL(policy_heads_wgrad_reduce_kernel, dim3((unsigned)((s.goff[kPhMatrices] + 255) / 256)), dim3(256), 0, st, r);
    return launched();
}

}  // extern "C"
