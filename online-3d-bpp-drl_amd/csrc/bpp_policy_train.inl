// bpp_policy_train.inl -- the training pass of the CNNPro trunk (include/bpp_policy_train.h), included at the end
// of bpp_kernels.hip after bpp_policy.inl: the forward that keeps its activations, the gradient at the pre-activation output of
// every layer, and the gradient of every trunk weight, float32 on the matrix cores.
//
// Forward: policy_trunk_kernel<true> (bpp_policy.inl), the inference kernel with one more store per layer.
//
// policy_trunk_grad_kernel: its sibling on the second blob.  The same two LDS images per bin, the same tables.  The masked head
// gradient gf' is staged as 20 channels, D5 = gf' x W_head^T is one product with K = 20, and every layer below is
// the forward's 3x3 product on the flipped and transposed weights, started from +0.  After a layer's product the image holds D;
// one pass over it reads the stored activation, applies the mask, and writes G to the image and to `grads` in rows.
//
// policy_wgrad_kernel: kfac_partial_kernel's sibling with two staged operands.  A workgroup of four waves owns 64 rows k of one
// layer's [K + 1][OC] gradient (a wave one 32 x 32 tile of the 2 x 2) and one split of the bins.  Per bin it stages the channels
// its 64 features touch of the layer's input, with their zero halo, and the layer's G [OC][A]; the MFMA's A operand is read at
// `offset of the feature + offset of the position`, the B operand at `offset of the output channel + position`.  Row K is the
// bias: a plane of ones staged behind the channels, so db is the chain fmaf(1, g, acc).  The partial tiles go to the workspace;
// policy_wgrad_reduce_kernel adds them per element in split order in double and casts once.
//
// The tile -- accumulator, layout, the instruction and its emulated chain -- is bpp_mfma.inl's.  g++ compiles this file too (tests/emu); nothing in it differs between the two builds.

namespace {

constexpr int kPtLayers = 6;                      // share.0 .. share.8 and the head convolutions
constexpr int kPtBlock = 2 * kPolTile;            // rows k (and columns oc) of a workgroup
constexpr int kPtChainRows = 1024;                // rows of a split aimed at
constexpr int kPtMaxSplitBins = 64;
constexpr int kPtBwdLayer = kPolTrunkK * kPolC;   // floats of one layer of weights_bwd

struct PtShape {
    PolShape p;
    int bps, splits, blocks, GS, wg_lds;          // bins per split, splits, 64-row blocks of all layers, floats between two staged G channels
    int blk0[kPtLayers + 1];                      // first block of a layer
};

struct PtGradArgs {
    const float *feat, *acts, *grad_feat, *wb;
    float *grads;
    PolShape s;
};

struct PtWgradArgs {
    const float *obs;
    long long obs_stride;
    const float *acts, *grads;
    float *part;
    PtShape s;
};

__host__ __device__ __forceinline__ int pt_channels(int layer) { return layer == 0 ? kPolIn : kPolC; }
__host__ __device__ __forceinline__ int pt_taps(int layer) { return layer == 5 ? 1 : 9; }
__host__ __device__ __forceinline__ int pt_outputs(int layer) { return layer == 5 ? kPolHeadC : kPolC; }
__host__ __device__ __forceinline__ int pt_rows(int layer) { return pt_channels(layer) * pt_taps(layer) + 1; }     // K + 1: the bias row

// grid = ceil(n / P)
__global__ __launch_bounds__(256) void policy_trunk_grad_kernel(PtGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PolShape &s = a.s;
    float *src = (float *)smem, *dst = src + s.P * s.img;
    int *ftab = (int *)(dst + s.P * s.img);
    int *rtab = ftab + kPolTrunkK;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31;
    const long long bin0 = (long long)blockIdx.x * s.P;
    const int CA = kPolC * s.A, F = kPolHeadC * s.A, centre = s.PW + 1;
    for (int idx = tid; idx < 2 * s.P * s.img; idx += 256) src[idx] = 0.0f;
    for (int k = tid; k < kPolTrunkK; k += 256) {
        const int c = k / 9, q = k - c * 9, i = q / 3;
        ftab[k] = c * s.PP + i * s.PW + (q - i * 3);
    }
    for (int r = tid; r < s.tiles * kPolTile; r += 256) {
        const int b = r / s.A, p = r - b * s.A, y = p / s.S;
        rtab[r] = r < s.rows ? b * s.img + y * s.PW + (p - y * s.S) : 0;
    }
    __syncthreads();
    // gf' = feat > 0 ? grad_feat : 0 as 20 channels of src, and to the sixth array of grads
    float *ghead = a.grads + (size_t)5 * (size_t)s.n * (size_t)CA;
    for (int idx = tid; idx < s.P * F; idx += 256) {
        const int b = idx / F, rem = idx - b * F, h = rem / s.A, p = rem - h * s.A, y = p / s.S;
        if (bin0 + b < s.n) {
            const size_t at = (size_t)(bin0 + b) * (size_t)F + (size_t)rem;
            const float g = a.feat[at] > 0.0f ? a.grad_feat[at] : 0.0f;
            src[b * s.img + h * s.PP + y * s.PW + (p - y * s.S) + centre] = g;
            ghead[at] = g;
        }
    }
    __syncthreads();
    for (int layer = 4; layer >= 0; --layer) {
        // D of trunk layer `layer` (0-based) from the G above it: the head product for layer 4, a flipped 3x3 product below
        for (int pt = wave; pt < s.tiles; pt += 4) {
            const int *rt = rtab + pt * kPolTile;
            const int ro = rt[col];
            MfmaAcc acc[2];
            mfma_fill(acc, [](int) { return 0.0f; });
            if (layer == 4)
                policy_chain<2, 5>(acc, src + centre, rt, ro, nullptr, s.PP, kPolHeadC, a.wb + (size_t)4 * kPtBwdLayer, kPolC, 0, kPolC, lane);
            else
                policy_chain<2, 9>(acc, src, rt, ro, ftab, 0, kPolTrunkK, a.wb + (size_t)layer * kPtBwdLayer, kPolC, 0, kPolC, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < kMfmaSlots; ++q) {
                    const int row = pt * kPolTile + mfma_slot_row(q, lane);
                    if (row < s.rows) dst[rtab[row] + (kPolTile * t + col) * s.PP + centre] = acc[t][q];
                }
            }
        }
        __syncthreads();
        // G = act > 0 ? D : 0, in place and to grads
        const float *act = a.acts + (size_t)layer * (size_t)s.n * (size_t)CA;
        float *out = a.grads + (size_t)layer * (size_t)s.n * (size_t)CA;
        for (int idx = tid; idx < s.P * CA; idx += 256) {
            const int b = idx / CA, rem = idx - b * CA, c = rem / s.A, p = rem - c * s.A, y = p / s.S;
            float *d = dst + b * s.img + c * s.PP + y * s.PW + (p - y * s.S) + centre;
            float g = 0.0f;
            if (bin0 + b < s.n) {
                const size_t at = (size_t)(bin0 + b) * (size_t)CA + (size_t)rem;
                g = act[at] > 0.0f ? *d : 0.0f;
                out[at] = g;
            }
            *d = g;
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
    }
}

// acc += A^T-by-B of rows r and r + 1 of the staged bin (row r + 1 counts as zeros when the bin ends at r):
// acc[i][j] = fmaf(x[r + 1][i], g[r + 1][j], fmaf(x[r][i], g[r][j], acc[i][j])), x[r][i] = img[ta[i] + rtab[r]] the patch value of
// feature i at position r, g[r][j] = gimg[tb[j] + r].  fa / fb: this lane's own ta[lane & 31] / tb[lane & 31].
__device__ __forceinline__ void policy_wgrad_mac(MfmaAcc &acc, const float *img, const float *gimg, const int *ta, const int *tb, int fa, int fb,
                                                 const int *rtab, int r, int nr, int lane) {
    const int k = r + (lane >> 5);                    // the lane's own operands, the only ones the device fetches
    const bool ok = k < nr;
    const int kk = ok ? k : r;
    const float x = ok ? img[fa + rtab[kk]] : 0.0f, b = ok ? gimg[fb + kk] : 0.0f;
    mfma_step(acc, lane, x, b, [&](int i, int q) { return r + q < nr ? img[ta[i] + rtab[r + q]] : 0.0f; },
              [&](int q, int j) { return r + q < nr ? gimg[tb[j] + r + q] : 0.0f; });
}

// grid = blocks x splits: workgroup g takes block g % blocks and split g / blocks
__global__ __launch_bounds__(256) void policy_wgrad_kernel(PtWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PtShape &s = a.s;
    const PolShape &p = s.p;
    float *img = (float *)smem;                           // the staged channels [<= 64][PP], the plane of ones among them
    float *gimg = img + kPolC * p.PP;                     // G of the bin [OC][GS]
    int *ftab = (int *)(gimg + kPolC * s.GS);             // [64] feature offsets, [64] output channel offsets
    int *rtab = ftab + 2 * kPtBlock;                      // [A]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int blk = (int)(blockIdx.x % (unsigned)s.blocks), split = (int)(blockIdx.x / (unsigned)s.blocks);
    int layer = 0;
    while (blk >= s.blk0[layer + 1]) ++layer;
    const int C = pt_channels(layer), KK = pt_taps(layer), OC = pt_outputs(layer), K1 = pt_rows(layer);
    const int f0 = (blk - s.blk0[layer]) * kPtBlock, f1 = min(K1, f0 + kPtBlock);
    const int c0 = f0 / KK, c1 = (f1 - 1) / KK + 1;       // the channels staged; channel C is the plane of ones
    const int centre = p.PW + 1, CA = kPolC * p.A;
    for (int idx = tid; idx < kPolC * p.PP; idx += 256) img[idx] = c0 + idx / p.PP == C ? 1.0f : 0.0f;
    if (tid < kPtBlock) {
        const int gf = f0 + tid;
        int off = 0;
        if (gf < K1) {
            const int c = gf / KK, q = gf - c * KK, i = q / 3;
            off = (c - c0) * p.PP + (KK == 1 ? centre : i * p.PW + (q - i * 3));
        }
        ftab[tid] = off;
    } else if (tid < 2 * kPtBlock) {
        const int oc = tid - kPtBlock;
        ftab[tid] = oc < OC ? oc * s.GS : 0;
    }
    for (int r = tid; r < p.A; r += 256) {
        const int y = r / p.S;
        rtab[r] = y * p.PW + (r - y * p.S);
    }
    __syncthreads();
    const int wi = wave >> 1, wj = wave & 1;
    // a tile with no row below K1 or no column below OC does nothing and writes nothing; inside an active tile the rows from K1
    // and the columns from OC on compute values the reduce kernel never reads
    const bool active = f0 + wi * kPolTile < K1 && wj * kPolTile < OC;
    const int *ta = ftab + wi * kPolTile, *tb = ftab + kPtBlock + wj * kPolTile;
    const int fa = ta[lane & 31], fb = tb[lane & 31];
    MfmaAcc acc;
#pragma unroll
    for (int k = 0; k < kMfmaSlots; ++k) acc[k] = 0.0f;
    const float *x = layer == 0 ? a.obs : a.acts + (size_t)(layer == 5 ? 4 : layer - 1) * (size_t)p.n * (size_t)CA;
    const size_t xstride = layer == 0 ? (size_t)a.obs_stride : (size_t)CA;
    const float *g = a.grads + (size_t)layer * (size_t)p.n * (size_t)CA;
    const int nc = min(c1, C) - c0, GA = OC * p.A;
    const long long b0 = (long long)split * s.bps, b1 = min((long long)p.n, b0 + s.bps);
    for (long long b = b0; b < b1; ++b) {
        const float *xb = x + (size_t)b * xstride + (size_t)c0 * (size_t)p.A;
        for (int idx = tid; idx < nc * p.A; idx += 256) {
            const int c = idx / p.A, q = idx - c * p.A, y = q / p.S;
            img[c * p.PP + y * p.PW + (q - y * p.S) + centre] = xb[idx];
        }
        const float *gb = g + (size_t)b * (size_t)GA;
        for (int idx = tid; idx < GA; idx += 256) {
            const int oc = idx / p.A;
            gimg[oc * s.GS + (idx - oc * p.A)] = gb[idx];
        }
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int r = 0; r < p.A; r += 2) policy_wgrad_mac(acc, img, gimg, ta, tb, fa, fb, rtab, r, p.A, lane);
        }
        __syncthreads();
    }
    if (active) {
        float *out = a.part + (((size_t)split * (size_t)s.blocks + (size_t)blk) * 4u + (size_t)wave) * 1024u;
#pragma unroll
        for (int k = 0; k < kMfmaSlots; ++k) out[k * kWave + lane] = acc[k];
    }
}

// One lane per float of grad_weights: the partials of the splits in order, in double, cast once.
__global__ __launch_bounds__(256) void policy_wgrad_reduce_kernel(const float *part, float *gw, PtShape s) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= (int)s.p.w_lin[0][0]) return;
    int layer = 5;
    while (layer > 0 && e < (int)(layer == 5 ? s.p.w_head_conv : s.p.w_conv[layer])) --layer;
    const int OC = pt_outputs(layer), idx = e - (int)(layer == 5 ? s.p.w_head_conv : s.p.w_conv[layer]);
    const int k = idx / OC, oc = idx - k * OC;
    const int blk = s.blk0[layer] + k / kPtBlock, wave = 2 * ((k % kPtBlock) / kPolTile) + oc / kPolTile;
    const size_t stride = (size_t)s.blocks * 4096u;
    const float *at = part + ((size_t)blk * 4u + (size_t)wave) * 1024u + (size_t)mfma_stored_at(k % kPolTile, oc % kPolTile);
    double sum = 0.0;
    for (int sp = 0; sp < s.splits; ++sp) sum = sum + (double)at[(size_t)sp * stride];
    gw[e] = (float)sum;
}

int policy_train_shape(const int32_t *g, int32_t n, const ArgCheck &ck, PtShape &s) {
    if (const int rc = policy_shape(g, n, true, ck, s.p)) return rc;
    const PolShape &p = s.p;
    s.bps = max(1, min(kPtMaxSplitBins, kPtChainRows / p.A));
    const long long splits = ((long long)n + s.bps - 1) / s.bps;
    s.blk0[0] = 0;
    for (int l = 0; l < kPtLayers; ++l) s.blk0[l + 1] = s.blk0[l] + (pt_rows(l) + kPtBlock - 1) / kPtBlock;
    s.blocks = s.blk0[kPtLayers];
    if (splits * s.blocks > 2147483647LL) return ck.bad("n too large");
    s.splits = (int)splits;
    s.GS = p.A | 1;
    s.wg_lds = (kPolC * p.PP + kPolC * s.GS + 2 * kPtBlock + p.A) * 4;
    if (s.wg_lds > kPolLdsBytes) return ck.bad("the staged operands of a bin do not fit the LDS");
    return 0;
}

size_t policy_train_workspace(const PtShape &s) { return (size_t)s.splits * (size_t)s.blocks * 4096u * sizeof(float); }

}  // namespace

extern "C" {

size_t bpp_policy_trunk_backward_workspace(const int32_t geom[], int32_t n) {
    PtShape s;
    if (policy_train_shape(geom, n, ArgCheck{"bpp_policy_trunk_backward_workspace"}, s)) return 0;
    return policy_train_workspace(s);
}

size_t bpp_policy_trunk_backward_weights_floats(const int32_t geom[]) {
    PolShape s;
    if (policy_shape(geom, 0, false, ArgCheck{"bpp_policy_trunk_backward_weights_floats"}, s)) return 0;
    return (size_t)4 * kPtBwdLayer + (size_t)kPolHeadC * kPolC;
}

int bpp_policy_trunk_backward_info(const int32_t geom[], int32_t n, int32_t out[8]) {
    const ArgCheck ck{"bpp_policy_trunk_backward_info"};
    PtShape s;
    if (out) out[6] = 0;
    if (const int rc = policy_train_shape(geom, n, ck, s)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = s.p.P, out[1] = s.p.trunk_lds, out[2] = s.bps, out[3] = s.splits, out[4] = min(s.bps, n) * s.p.A, out[5] = s.wg_lds;
    out[6] = 1, out[7] = s.blocks;
    return 0;
}

int bpp_policy_trunk_forward_train(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *feat,
                                   float *acts, void *stream) {
    const ArgCheck ck{"bpp_policy_trunk_forward_train"};
    if (!obs || !geom || !weights || !feat || !acts) return ck.bad("NULL pointer");
    PolTrunkArgs t;
    if (const int rc = policy_shape(geom, n, true, ck, t.s)) return rc;
    if (obs_stride < (int64_t)kPolIn * t.s.A) return ck.bad("obs_stride must be >= 4 A");
    const PolShape &s = t.s;
    t.obs = obs, t.obs_stride = obs_stride, t.w = weights, t.feat = feat, t.acts = acts;
    return launch_large_lds<policy_trunk_kernel<true>>(dim3((unsigned)(((long long)n + s.P - 1) / s.P)), dim3(256), s.trunk_lds, kPolLdsBytes,
                                                       (hipStream_t)stream, t);
}

int bpp_policy_trunk_backward(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights_bwd, const float *feat,
                              const float *acts, const float *grad_feat, float *grads, float *grad_weights, void *workspace,
                              size_t workspace_bytes, void *stream) {
    const ArgCheck ck{"bpp_policy_trunk_backward"};
    if (!obs || !geom || !weights_bwd || !feat || !acts || !grad_feat || !grads || !grad_weights || !workspace) return ck.bad("NULL pointer");
    PtWgradArgs w;
    if (const int rc = policy_train_shape(geom, n, ck, w.s)) return rc;
    const PtShape &s = w.s;
    if (obs_stride < (int64_t)kPolIn * s.p.A) return ck.bad("obs_stride must be >= 4 A");
    if (workspace_bytes < policy_train_workspace(s)) return ck.bad("workspace smaller than bpp_policy_trunk_backward_workspace");
    const hipStream_t st = (hipStream_t)stream;
    PtGradArgs g;
    g.feat = feat, g.acts = acts, g.grad_feat = grad_feat, g.wb = weights_bwd, g.grads = grads, g.s = s.p;
    if (const int rc = launch_large_lds<policy_trunk_grad_kernel>(dim3((unsigned)(((long long)n + s.p.P - 1) / s.p.P)), dim3(256), s.p.trunk_lds,
                                                                  kPolLdsBytes, st, g))
        return rc;
    w.obs = obs, w.obs_stride = obs_stride, w.acts = acts, w.grads = grads, w.part = (float *)workspace;
    if (const int rc = launch_large_lds<policy_wgrad_kernel>(dim3((unsigned)s.blocks * (unsigned)s.splits), dim3(256), s.wg_lds, kPolLdsBytes, st, w))
        return rc;
    const int floats = (int)s.p.w_lin[0][0];
    hipLaunchKernelGGL(policy_wgrad_reduce_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, st, (const float *)workspace, grad_weights,
                       s);
    return launched();
}

}  // extern "C"
