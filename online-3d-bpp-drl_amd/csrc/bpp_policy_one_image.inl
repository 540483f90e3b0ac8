// bpp_policy_one_image.inl -- the policy forward on ONE LDS image per bin (include/bpp_policy_one_image.h),
// included in bpp_kernels.hip behind bpp_policy.inl, whose shapes, chain (policy_chain, policy_start) and head kernel it uses.
//
// policy_trunk_one_image_kernel<TW>: a workgroup of four waves owns P bins and one image [64][PP] per bin.  Wave w owns the
// position tiles w, w + 4, .. (TW of them at most).  A layer: the wave runs the whole k chain of each of its tiles and keeps
// the outputs in acc[TW][2]; behind a barrier -- nobody reads the image any more -- it writes ReLU(acc) into the interior of the
// image it read from; a second barrier, and the image is the next layer's input.  The halo is zeroed once and never written.
// The head convolutions go the same way into acc[TW][1]; their features [P][20 A] overwrite the start of the image.
//
// TW is a template parameter and every index into the accumulators is unrolled: they stay in registers (128 of them at TW = 4).
// g++ compiles this file too (tests/emu).

namespace {

template <int TW>
__global__ __launch_bounds__(256, TW <= 2 ? 2 : 1) void policy_trunk_one_image_kernel(PolTrunkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const PolShape &s = a.s;
    float *img = (float *)smem;                       // [P][64][PP]
    int *ftab = (int *)(img + s.P * s.img);           // [576]: where feature k of a 3x3 layer lies, from the patch's corner
    int *rtab = ftab + kPolTrunkK;                    // [tiles * 32]: the patch corner of position row r (a row beyond `rows`: 0)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, col = lane & 31;
    const long long bin0 = (long long)blockIdx.x * s.P;
    for (int idx = tid; idx < s.P * s.img; idx += 256) img[idx] = 0.0f;
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
            img[b * s.img + c * s.PP + (y + 1) * s.PW + (p - y * s.S) + 1] = a.obs[(size_t)(bin0 + b) * (size_t)a.obs_stride + (size_t)rem];
    }
    __syncthreads();
    const int centre = s.PW + 1;                      // from a patch's corner to its position
    for (int layer = 0; layer < 5; ++layer) {
        const int K = layer ? kPolTrunkK : kPolIn * 9;
        const float *w = a.w + s.w_conv[layer], *bias = w + K * kPolC;
        MfmaAcc acc[TW][2];
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            const int pt = wave + 4 * j;
            if (pt < s.tiles) {
                const int *rt = rtab + pt * kPolTile;
                policy_start<2>(acc[j], bias, 0, kPolC, lane);
                policy_chain<2, 9>(acc[j], img, rt, rt[col], ftab, 0, K, w, kPolC, 0, kPolC, lane);
            }
        }
        __syncthreads();                              // every chain of the layer has read what it needs of the image
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            const int pt = wave + 4 * j;
            if (pt < s.tiles) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int q = 0; q < kMfmaSlots; ++q) {
                        const int row = pt * kPolTile + mfma_slot_row(q, lane);
                        const float v = acc[j][t][q];
                        if (row < s.rows) img[rtab[row] + (kPolTile * t + col) * s.PP + centre] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
    }
    // the three 1x1 head convolutions as one product with 20 columns; [P][20 A] at the start of the image behind the barrier
    const float *w = a.w + s.w_head_conv, *bias = w + kPolC * kPolHeadC;
    const int F = kPolHeadC * s.A;
    MfmaAcc acc[TW][1];
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int pt = wave + 4 * j;
        if (pt < s.tiles) {
            const int *rt = rtab + pt * kPolTile;
            policy_start<1>(acc[j], bias, 0, kPolHeadC, lane);
            policy_chain<1, 8>(acc[j], img + centre, rt, rt[col], nullptr, s.PP, kPolC, w, kPolHeadC, 0, kPolHeadC, lane);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int pt = wave + 4 * j;
        if (pt < s.tiles) {
#pragma unroll
            for (int q = 0; q < kMfmaSlots; ++q) {
                const int row = pt * kPolTile + mfma_slot_row(q, lane);
                const float v = acc[j][0][q];
                if (row < s.rows && col < kPolHeadC) {
                    const int b = row / s.A;
                    img[b * F + col * s.A + (row - b * s.A)] = v > 0.0f ? v : 0.0f;
                }
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < s.P * F; idx += 256)
        if (bin0 + idx / F < s.n) a.feat[(size_t)bin0 * (size_t)F + (size_t)idx] = img[idx];
}

int policy_one_image_tiles_per_wave(const PolShape &s) { return (s.tiles + 3) / 4; }

template <int TW>
int launch_policy_trunk_one_image(const PolTrunkArgs &t, hipStream_t st) {
    return launch_large_lds<policy_trunk_one_image_kernel<TW>>(dim3((unsigned)(((long long)t.s.n + t.s.P - 1) / t.s.P)), dim3(256), t.s.trunk_lds,
                                                               kPolLdsBytes, st, t);
}

}  // namespace

extern "C" {

size_t bpp_policy_forward_one_image_workspace(const int32_t geom[], int32_t n) {
    PolShape s;
    if (policy_shape(geom, n, true, ArgCheck{"bpp_policy_forward_one_image_workspace"}, s, 1)) return 0;
    return (size_t)n * (size_t)(kPolHeadC * s.A) * sizeof(float);
}

size_t bpp_policy_one_image_weights_floats(const int32_t geom[]) {
    PolShape s;
    if (policy_shape(geom, 0, false, ArgCheck{"bpp_policy_one_image_weights_floats"}, s, 1)) return 0;
    return (size_t)s.total;
}

int bpp_policy_forward_one_image_info(const int32_t geom[], int32_t n, int32_t out[8]) {
    const ArgCheck ck{"bpp_policy_forward_one_image_info"};
    PolShape s;
    if (out) out[7] = 0;
    if (const int rc = policy_shape(geom, n, true, ck, s, 1)) return rc;
    if (!out) return ck.bad("NULL out");
    out[0] = s.P, out[1] = s.trunk_lds, out[2] = (int32_t)(((long long)n + s.P - 1) / s.P), out[3] = policy_one_image_tiles_per_wave(s);
    out[4] = 3 * (int32_t)(((long long)n + kPolT - 1) / kPolT), out[5] = kPolTile, out[6] = s.tiles * kPolTile, out[7] = 2;
    return 0;
}

int bpp_policy_forward_one_image(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *value,
                                 float *logits, float *pred, void *workspace, void *stream) {
    const ArgCheck ck{"bpp_policy_forward_one_image"};
    if (!obs || !geom || !weights || !workspace) return ck.bad("NULL pointer");
    if (!value && !logits && !pred) return ck.bad("at least one of value, logits and pred must be asked for");
    PolTrunkArgs t;
    if (const int rc = policy_shape(geom, n, true, ck, t.s, 1)) return rc;
    if (obs_stride < (int64_t)kPolIn * t.s.A) return ck.bad("obs_stride must be >= 4 A");
    const PolShape &s = t.s;
    const hipStream_t st = (hipStream_t)stream;
    t.obs = obs, t.obs_stride = obs_stride, t.w = weights, t.feat = (float *)workspace, t.acts = nullptr;
    int rc;
    switch (policy_one_image_tiles_per_wave(s)) {
        case 1: rc = launch_policy_trunk_one_image<1>(t, st); break;
        case 2: rc = launch_policy_trunk_one_image<2>(t, st); break;
        case 3: rc = launch_policy_trunk_one_image<3>(t, st); break;
        case 4: rc = launch_policy_trunk_one_image<4>(t, st); break;
        default: return ck.bad("more than 4 position tiles per wave");        // S <= 22 has 16 tiles at most
    }
    if (rc) return rc;
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
