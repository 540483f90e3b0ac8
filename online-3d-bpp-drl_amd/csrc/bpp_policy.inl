// bpp_policy.inl -- the CNNPro policy forward for inference (include/bpp_policy.h), included at the end of
// bpp_kernels.hip: acktr/model.py:265-323 and dist.linear (acktr/distributions.py:72) in float32 on the matrix cores.
//
// policy_trunk_kernel: a workgroup of four waves owns P bins.  Each bin has two images [64][PP] in LDS (PP = (S + 2)^2 made odd:
// the S x S plane of a channel inside a halo of zeros); the five 3x3 layers go back and forth between them.  A layer is the
// product [positions of the P bins] x [k = c * 9 + i * 3 + j] x [64 output channels] on v_mfma_f32_32x32x2_f32: a wave takes
// 32 positions at a time and both halves of the output channels, reads the A operand from the source image at `offset of the
// feature + offset of the position` (two small tables, as bpp_kfac.inl does) and the B operand from the packed weights, starts
// the accumulators at the bias and writes ReLU(acc) into the interior of the other image; the halo is zeroed once and never
// written.  The three 1x1 head convolutions are one more product with 20 columns; their output is collected in LDS and copied
// to the workspace in rows.  policy_head_kernel: a workgroup owns 64 bins and one head; the features pass through LDS 64 input
// features at a time, the hidden vector stays in LDS between the two Linear layers.
//
// The tile -- accumulator, layout, the instruction and its emulated chain -- is bpp_mfma.inl's.  g++ compiles this file too
// (tests/emu): policy_chain is the only function that differs, by the software-pipelined loop that only the device has.

namespace {

constexpr int kPolTile = kMfmaTile;
constexpr int kPolC = 64;                 // trunk channels
constexpr int kPolIn = 4;                 // input channels
constexpr int kPolHeadC = 20;             // actor 8 + mask 8 + critic 4
constexpr int kPolMaxBins = 2;            // bins of a trunk workgroup at most
constexpr int kPolT = 64;                 // bins of a head workgroup
constexpr int kPolChunk = 64;             // input features of a Linear staged at a time
constexpr int kPolStride = kPolT + 1;     // floats between two features of the staged chunk and of the hidden vector (odd)
constexpr int kPolMaxHidden = 512;
constexpr int kPolLdsBytes = 160 * 1024;
constexpr int kPolTrunkK = kPolC * 9;
constexpr int kPolOneImageMaxSide = 22;   // one image [64][(S + 2)^2 | 1] and the tables within kPolLdsBytes: 152 064 B at 22

struct PolShape {
    int S, H, M, A, PW, PP, img;          // img: floats of one image
    int P, tiles, rows, n;                // bins, position tiles and positions of a trunk workgroup
    int trunk_lds, head_lds;
    long long w_conv[5], w_head_conv, w_lin[3][2], total;       // offsets into the blob; w_lin[head]: actor, mask, critic
};

struct PolTrunkArgs {
    const float *obs;
    long long obs_stride;
    const float *w;
    float *feat;
    float *acts;                          // training forward only (bpp_policy_train.inl): five arrays [n][64][A]
    PolShape s;
};

struct PolHeadArgs {
    const float *feat;
    const float *w;
    float *out[3];                        // logits, pred, value
    float *hidden;                        // training forward only (bpp_policy_heads_train.inl): [3][n][H]
    int heads[3], nheads;
    PolShape s;
};

// One chain per output element over k = 0 .. K - 1 (K even), NB column tiles of 32 at once:
//   acc[t][r][c] = fmaf(A[r][k], B[k][col0 + 32 t + c], acc[t][r][c])    in ascending k
// A[r][k] = img[rt[r] + (ftab ? ftab[k] : k * kstride)], ro = rt[lane & 31]; B[k][c] = w[k * ldw + c].  A column from ncol on reads
// column ncol - 1 instead and its result is never used.  A table must repeat with period 2 U: ftab[k + 2 U] - ftab[k] is one
// constant (U = 9: two channels of a 3x3 layer).
//
// Two k go into one mfma_step (bpp_mfma.inl): lane l passes A[l & 31][k + (l >> 5)] and B[k + (l >> 5)][l & 31].  On the device
// the operands of U instructions per column tile are fetched while the U before them issue: with one wave per SIMD nothing else
// hides the latency of the weights.  What that loop leaves of K goes through the plain loop behind it; emulated, all of K does.
// Both walk k in pairs, so K must be even as stated above: every caller's is (36, 576, 64, 20, H, and 4 A or 8 A in chunks of 64;
// bpp_policy_heads_train.inl makes an odd chunk even with a row of zeros).
template <int NB, int U>
__device__ __forceinline__ void policy_chain(MfmaAcc (&acc)[NB], const float *img, const int *rt, int ro, const int *ftab, int kstride, int K,
                                             const float *__restrict__ w, int ldw, int col0, int ncol, int lane) {
    const int col = lane & 31, half = lane >> 5;
    const auto column = [&](int t, int j) { return min(col0 + kPolTile * t + j, ncol - 1); };
    int cc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) cc[t] = column(t, col);
    const float *ap = img + ro;
    int k0 = 0;
#ifndef BPP_EMU_HIP_RUNTIME_H
    int off[U];
#pragma unroll
    for (int u = 0; u < U; ++u) off[u] = ftab ? ftab[2 * u + half] : (2 * u + half) * kstride;
    const int adv = ftab ? ftab[2 * U] - ftab[0] : 2 * U * kstride;
    const int nb = K / (2 * U);
    const float *__restrict__ wp = w + (size_t)half * (size_t)ldw;
    float a0[U], b0[U][NB];
    if (nb > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a0[u] = ap[off[u]];
#pragma unroll
            for (int t = 0; t < NB; ++t) b0[u][t] = wp[(size_t)(2 * u) * (size_t)ldw + (size_t)cc[t]];
        }
    }
    for (int i = 0; i < nb; ++i) {
        const int nx = min(i + 1, nb - 1);              // the last batch fetches itself again: no branch in the loop
        const float *an = ap + nx * adv;
        const float *__restrict__ wn = wp + (size_t)nx * (size_t)(2 * U) * (size_t)ldw;
        float a1[U], b1[U][NB];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a1[u] = an[off[u]];
#pragma unroll
            for (int t = 0; t < NB; ++t) b1[u][t] = wn[(size_t)(2 * u) * (size_t)ldw + (size_t)cc[t]];
        }
        __builtin_amdgcn_sched_barrier(0);              // the fetches stay in front of the MFMAs they overlap with
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int t = 0; t < NB; ++t) mfma_issue(acc[t], a0[u], b0[u][t]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            asm volatile("" : "+v"(a1[u]));             // the value that was fetched, not a second load next to its use
            a0[u] = a1[u];
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                asm volatile("" : "+v"(b1[u][t]));
                b0[u][t] = b1[u][t];
            }
        }
    }
    k0 = nb * 2 * U;
#endif
    const auto koff = [&](int k) { return ftab ? ftab[k] : k * kstride; };
    for (int k = k0 + half; k < K; k += 2) {
        const float a = ap[koff(k)];
#pragma unroll
        for (int t = 0; t < NB; ++t)
            mfma_step(acc[t], lane, a, w[(size_t)k * (size_t)ldw + (size_t)cc[t]],
                      [&](int i, int kk) { return img[rt[i] + koff(k - half + kk)]; },
                      [&](int kk, int j) { return w[(size_t)(k - half + kk) * (size_t)ldw + (size_t)column(t, j)]; });
    }
}

// every slot of acc[t] = bias of the lane's column (0 from column ncol on): the chain starts from the bias
template <int NB>
__device__ __forceinline__ void policy_start(MfmaAcc (&acc)[NB], const float *bias, int col0, int ncol, int lane) {
    mfma_fill(acc, [&](int t) {
        const int c = col0 + kPolTile * t + (lane & 31);
        return c < ncol ? bias[c] : 0.0f;
    });
}

// grid = ceil(n / P).  ACTS: every layer's ReLU output also goes to a.acts, copied from the image it was written to.
template <bool ACTS>
__global__ __launch_bounds__(256) void policy_trunk_kernel(PolTrunkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PolShape &s = a.s;
    float *src = (float *)smem, *dst = src + s.P * s.img;
    int *ftab = (int *)(dst + s.P * s.img);           // [576]: where feature k of a 3x3 layer lies, from the patch's corner
    int *rtab = ftab + kPolTrunkK;                    // [tiles * 32]: the patch corner of position row r (a row beyond `rows`: 0)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31;
    const long long bin0 = (long long)blockIdx.x * s.P;
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
    for (int idx = tid; idx < s.P * kPolIn * s.A; idx += 256) {
        const int b = idx / (kPolIn * s.A), rem = idx - b * (kPolIn * s.A), c = rem / s.A, p = rem - c * s.A, y = p / s.S;
        if (bin0 + b < s.n)
            src[b * s.img + c * s.PP + (y + 1) * s.PW + (p - y * s.S) + 1] = a.obs[(size_t)(bin0 + b) * (size_t)a.obs_stride + (size_t)rem];
    }
    __syncthreads();
    const int centre = s.PW + 1;                      // from a patch's corner to its position
    for (int layer = 0; layer < 5; ++layer) {
        const int K = layer ? kPolTrunkK : kPolIn * 9;
        const float *w = a.w + s.w_conv[layer], *bias = w + K * kPolC;
        for (int pt = wave; pt < s.tiles; pt += 4) {
            const int *rt = rtab + pt * kPolTile;
            const int ro = rt[col];
            MfmaAcc acc[2];
            policy_start<2>(acc, bias, 0, kPolC, lane);
            policy_chain<2, 9>(acc, src, rt, ro, ftab, 0, K, w, kPolC, 0, kPolC, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < kMfmaSlots; ++q) {
                    const int row = pt * kPolTile + mfma_slot_row(q, lane);
                    const float v = acc[t][q];
                    if (row < s.rows) dst[rtab[row] + (kPolTile * t + col) * s.PP + centre] = v > 0.0f ? v : 0.0f;
                }
            }
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
        if (ACTS) {
            float *out = a.acts + (size_t)layer * (size_t)s.n * (size_t)(kPolC * s.A);
            for (int idx = tid; idx < s.P * kPolC * s.A; idx += 256) {
                const int b = idx / (kPolC * s.A), rem = idx - b * (kPolC * s.A), c = rem / s.A, p = rem - c * s.A, y = p / s.S;
                if (bin0 + b < s.n) out[(size_t)(bin0 + b) * (size_t)(kPolC * s.A) + (size_t)rem] = src[b * s.img + c * s.PP + y * s.PW + (p - y * s.S) + centre];
            }
        }
    }
    // the three 1x1 head convolutions as one product with 20 columns; dst is free now and collects [P][20 A]
    const float *w = a.w + s.w_head_conv, *bias = w + kPolC * kPolHeadC;
    const int F = kPolHeadC * s.A;
    for (int pt = wave; pt < s.tiles; pt += 4) {
        const int *rt = rtab + pt * kPolTile;
        const int ro = rt[col];
        MfmaAcc acc[1];
        policy_start<1>(acc, bias, 0, kPolHeadC, lane);
        policy_chain<1, 8>(acc, src + centre, rt, ro, nullptr, s.PP, kPolC, w, kPolHeadC, 0, kPolHeadC, lane);
#pragma unroll
        for (int q = 0; q < kMfmaSlots; ++q) {
            const int row = pt * kPolTile + mfma_slot_row(q, lane);
            const float v = acc[0][q];
            if (row < s.rows && col < kPolHeadC) {
                const int b = row / s.A;
                dst[b * F + col * s.A + (row - b * s.A)] = v > 0.0f ? v : 0.0f;
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < s.P * F; idx += 256)
        if (bin0 + idx / F < s.n) a.feat[(size_t)bin0 * (size_t)F + (size_t)idx] = dst[idx];
}

// grid = ceil(n / 64) * heads asked for: workgroup g takes bin tile g / heads and head g % heads.  HID: the hidden vector also
// goes to a.hidden in rows, copied from the LDS it was written to.
template <bool HID>
__global__ __launch_bounds__(256) void policy_head_kernel(PolHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PolShape &s = a.s;
    float *hid = (float *)smem;                       // [H][65]: hidden feature h of bin b at h * 65 + b
    float *chunk = hid + s.H * kPolStride;            // [64][65]: the staged input features, the same way
    int *itab = (int *)(chunk + kPolChunk * kPolStride);      // [64]: row r of the tile is bin r
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31;
    const int head = a.heads[blockIdx.x % (unsigned)a.nheads];            // 0 actor -> logits, 1 mask -> pred, 2 critic -> value
    const int K1 = (head == 2 ? 4 : 8) * s.A, f0 = head * 8 * s.A, Mh = head == 2 ? 1 : s.M, F = kPolHeadC * s.A;
    const float *w1 = a.w + s.w_lin[head][0], *b1 = w1 + (size_t)K1 * (size_t)s.H;
    const float *w2 = a.w + s.w_lin[head][1], *b2 = w2 + (size_t)s.H * (size_t)Mh;
    const long long bin0 = (long long)(blockIdx.x / (unsigned)a.nheads) * kPolT;
    if (tid < kPolT) itab[tid] = tid;
    const int rtile = wave & 1, cgroup = wave >> 1;
    const int *rt = itab + rtile * kPolTile;
    const int ro = rtile * kPolTile + col;
    // first Linear: a pass covers 256 hidden features, a wave 32 bins by 128 of them
    for (int h0 = 0; h0 < s.H; h0 += 8 * kPolTile) {
        const int col0 = h0 + cgroup * 4 * kPolTile;
        MfmaAcc acc[4];
        policy_start<4>(acc, b1, col0, s.H, lane);
        for (int k0 = 0; k0 < K1; k0 += kPolChunk) {
            const int kc = min(kPolChunk, K1 - k0);
            for (int idx = tid; idx < kPolT * kc; idx += 256) {
                const int b = idx / kc, kk = idx - b * kc;
                chunk[kk * kPolStride + b] = bin0 + b < s.n ? a.feat[(size_t)(bin0 + b) * (size_t)F + (size_t)(f0 + k0 + kk)] : 0.0f;
            }
            __syncthreads();
            if (col0 < s.H) policy_chain<4, 8>(acc, chunk, rt, ro, nullptr, kPolStride, kc, w1 + (size_t)k0 * (size_t)s.H, s.H, col0, s.H, lane);
            __syncthreads();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = col0 + kPolTile * t + col;
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q) {
                const float v = acc[t][q];
                if (c < s.H) hid[c * kPolStride + rtile * kPolTile + mfma_slot_row(q, lane)] = v > 0.0f ? v : 0.0f;
            }
        }
    }
    __syncthreads();
    if (HID) {
        float *out = a.hidden + ((size_t)head * (size_t)s.n + (size_t)bin0) * (size_t)s.H;
        for (int idx = tid; idx < kPolT * s.H; idx += 256) {
            const int b = idx / s.H;
            if (bin0 + b < s.n) out[idx] = hid[(idx - b * s.H) * kPolStride + b];
        }
    }
    // second Linear: a wave takes 32 bins by 64 outputs at a time
    float *out = a.out[head];
    for (int col0 = cgroup * 2 * kPolTile; col0 < Mh; col0 += 4 * kPolTile) {
        MfmaAcc acc[2];
        policy_start<2>(acc, b2, col0, Mh, lane);
        policy_chain<2, 8>(acc, hid, rt, ro, nullptr, kPolStride, s.H, w2, Mh, col0, Mh, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int c = col0 + kPolTile * t + col;
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q) {
                const long long bin = bin0 + rtile * kPolTile + mfma_slot_row(q, lane);
                const float v = acc[t][q];
                if (c < Mh && bin < s.n) out[(size_t)bin * (size_t)Mh + (size_t)c] = head == 1 && !(v > 0.0f) ? 0.0f : v;
            }
        }
    }
}

// images: the LDS images a bin has in the trunk kernel -- 2 for policy_trunk_kernel and the training kernels, 1 for
// policy_trunk_one_image_kernel (bpp_policy_one_image.inl), which takes two bins only while its workgroup stays within half the LDS.
int policy_shape(const int32_t *g, int32_t n, bool need_n, const ArgCheck &ck, PolShape &s, int images = 2) {
    if (!g) return ck.bad("NULL geom");
    memset(&s, 0, sizeof s);
    s.S = g[0], s.H = g[1], s.M = g[2], s.n = n;
    if (s.S < 1 || s.H < 1) return ck.bad("S and H must be >= 1");
    if (images == 2 && s.S > 15) return ck.bad("the two images of a bin do not fit the LDS (S > 15)");
    if (s.S > kPolOneImageMaxSide) return ck.bad("the image of a bin does not fit the LDS (S > 22)");
    s.A = s.S * s.S;
    if (s.M != s.A && s.M != 2 * s.A) return ck.bad("M must be A or 2 A");
    if (s.H % kPolTile != 0 || s.H > kPolMaxHidden) return ck.bad("H must be a multiple of 32 and at most 512");
    if (need_n && n < 1) return ck.bad("n must be >= 1");
    s.PW = s.S + 2, s.PP = (s.PW * s.PW) | 1, s.img = kPolC * s.PP;
    for (s.P = kPolMaxBins; s.P >= 1; --s.P) {
        s.rows = s.P * s.A, s.tiles = (s.rows + kPolTile - 1) / kPolTile;
        s.trunk_lds = (images * s.P * s.img + kPolTrunkK + s.tiles * kPolTile) * 4;
        if (s.trunk_lds <= (images == 1 && s.P > 1 ? kPolLdsBytes / 2 : kPolLdsBytes)) break;
    }
    if (s.P < 1) return ck.bad("the images of a bin do not fit the LDS");
    s.head_lds = ((s.H + kPolChunk) * kPolStride + kPolT) * 4;
    long long at = 0;
    for (int l = 0; l < 5; ++l) {
        s.w_conv[l] = at;
        at += ((l ? kPolTrunkK : kPolIn * 9) + 1) * kPolC;
    }
    s.w_head_conv = at;
    at += (kPolC + 1) * kPolHeadC;
    for (int h = 0; h < 3; ++h) {
        const long long K1 = (h == 2 ? 4 : 8) * s.A, Mh = h == 2 ? 1 : s.M;
        s.w_lin[h][0] = at;
        at += (K1 + 1) * s.H;
        s.w_lin[h][1] = at;
        at += (s.H + 1) * Mh;
    }
    s.total = at;
    return 0;
}

}  // namespace

extern "C" {

size_t bpp_policy_forward_workspace(const int32_t geom[], int32_t n) {
    PolShape s;
    if (policy_shape(geom, n, true, ArgCheck{"bpp_policy_forward_workspace"}, s)) return 0;
    return (size_t)n * (size_t)(kPolHeadC * s.A) * sizeof(float);
}

size_t bpp_policy_weights_floats(const int32_t geom[]) {
    PolShape s;
    if (policy_shape(geom, 0, false, ArgCheck{"bpp_policy_weights_floats"}, s)) return 0;
    return (size_t)s.total;
}

int bpp_policy_forward_info(const int32_t geom[], int32_t n, int32_t out[8]) {
    const ArgCheck ck{"bpp_policy_forward_info"};
    PolShape s;
    if (out) out[7] = 0;
    if (const int rc = policy_shape(geom, n, true, ck, s)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = s.P, out[1] = s.trunk_lds, out[2] = (int32_t)(((long long)n + s.P - 1) / s.P), out[3] = kPolT;
    out[4] = 3 * (int32_t)(((long long)n + kPolT - 1) / kPolT), out[5] = kPolTile, out[6] = s.tiles * kPolTile, out[7] = 1;
    return 0;
}

int bpp_policy_forward(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *value,
                       float *logits, float *pred, void *workspace, void *stream) {
    const ArgCheck ck{"bpp_policy_forward"};
    if (!obs || !geom || !weights || !workspace) return ck.bad("NULL pointer");
    if (!value && !logits && !pred) return ck.bad("at least one of value, logits and pred must be asked for");
    PolTrunkArgs t;
    if (const int rc = policy_shape(geom, n, true, ck, t.s)) return rc;
    if (obs_stride < (int64_t)kPolIn * t.s.A) return ck.bad("obs_stride must be >= 4 A");
    const PolShape &s = t.s;
    const hipStream_t st = (hipStream_t)stream;
    t.obs = obs, t.obs_stride = obs_stride, t.w = weights, t.feat = (float *)workspace, t.acts = nullptr;
    if (const int rc = launch_large_lds<policy_trunk_kernel<false>>(dim3((unsigned)(((long long)n + s.P - 1) / s.P)), dim3(256), s.trunk_lds,
                                                                    kPolLdsBytes, st, t))
        return rc;
    PolHeadArgs h;
    h.feat = (const float *)workspace, h.w = weights, h.hidden = nullptr, h.s = s, h.nheads = 0;
    h.out[0] = logits, h.out[1] = pred, h.out[2] = value;
    for (int k = 0; k < 3; ++k) {
        h.heads[k] = 0;
        if (h.out[k]) h.heads[h.nheads++] = k;
    }
    return launch_large_lds<policy_head_kernel<false>>(dim3((unsigned)(((long long)n + kPolT - 1) / kPolT) * (unsigned)h.nheads), dim3(256), s.head_lds,
                                                kPolLdsBytes, st, h);
}

}  // extern "C"
