// bpp_ppo.inl -- the native half of a PPO update (include/bpp_ppo.h), included by bpp_kernels.hip after
// bpp_update.inl: the normalised advantages of a rollout, the row gather of a mini-batch's observations, and the clipped loss of
// one mini-batch with its gradients in one pass.
//
// The loss kernel is bpp_a2c_loss's sibling and is built from its parts: the row is a LossRow (RegRow for M <= 512, MemRow beyond)
// through row_stats and row_terms of bpp_heads.inl, the mask-prediction term is pred_mask_row, the per-row terms are added by
// loss_rows and loss_sums (bpp_update.inl) in the shape a2c_shape gives.  What differs: the network's outputs are the B dense rows
// of a mini-batch while mask, action and the four per-row scalars of the rollout are read in place at row idx[b], and the weight of
// the log-probability depends on the log-probability itself (the ratio), so the statistics of the row come before its weights.

namespace {

constexpr int kPpoCols = 7;         // value term, action term, ent, bad, sq, ratio, clipped
constexpr int kAdvWidth = 256;      // lanes of a block of the advantage sums
constexpr int kAdvMaxBlocks = 1024;
constexpr int kGatherPart = 512;    // floats of a row one wave copies

struct PpoArgs {
    const float *logits, *values, *pred, *mask, *value_preds, *returns, *old, *adv;
    const int64_t *idx, *action;
    float *g_logits, *g_values, *g_pred, *rows;
    double *partial;
    int B, E, M, iters, clipped_value;
    float lo, hi, c, cB, c_v, g_ent, g_bad, c_p;
};

template <int NJ>
__device__ __forceinline__ void ppo_row(const PpoArgs &a, size_t b, int lane, float (&out)[kPpoCols]) {
    const int M = a.M;
    const size_t off = b * (size_t)M;
    const int64_t r = a.idx ? a.idx[b] : (int64_t)b;
    if (r < 0 || r >= (int64_t)a.E) {      // no row of the rollout: nothing of it is read, everything of the row is NaN
        const float nan = __builtin_nanf("");
        for (int k = lane; k < M; k += kWave) {
            a.g_logits[off + k] = nan;
            if (a.pred) a.g_pred[off + k] = nan;
        }
        if (lane == 0) a.g_values[b] = nan;
#pragma unroll
        for (int j = 0; j < kPpoCols; ++j) out[j] = nan;
        return;
    }
    const float *x = a.logits + off, *m = a.mask + (size_t)r * (size_t)M;
    LossRow<NJ> row(x, m, M, lane);
    const float s = a.pred ? pred_mask_row<NJ>(row, a.pred + off, a.g_pred + off, a.c_p) : 0.0f;
    const int64_t act = a.action[r];
    const float A = a.adv[r], old = a.old[r], vp = a.value_preds[r], R = a.returns[r], v = a.values[b];
    const RowStats st = row_stats(row);
    const float logp = action_logp(x, m, M, act, st);
    const float ratio = expf(logp - old);
    const float surr1 = ratio * A, surr2 = fminf(fmaxf(ratio, a.lo), a.hi) * A;
    const float g_ratio = surr1 <= surr2 ? A : 0.0f;
    const HeadGrad w{act, -(g_ratio * ratio) * a.cB, a.g_ent, a.g_bad};
    float h, bad;
    row_terms<true, true>(row, st, w, a.g_logits + off, h, bad);
    const float d = v - R;
    float vterm, g_v;
    if (a.clipped_value) {
        const float t = v - vp;
        const float e = (vp + fminf(fmaxf(t, -a.c), a.c)) - R;
        const float d2 = d * d, e2 = e * e;
        const float ep = e * ((t >= -a.c && t <= a.c) ? 1.0f : 0.0f);
        vterm = 0.5f * fmaxf(d2, e2);
        g_v = d2 > e2 ? d : d2 < e2 ? ep : 0.5f * d + 0.5f * ep;
    } else {
        vterm = 0.5f * (d * d);
        g_v = d;
    }
    if (lane == 0) a.g_values[b] = a.c_v * g_v;
    out[0] = vterm, out[1] = -fminf(surr1, surr2), out[2] = h, out[3] = bad, out[4] = s, out[5] = ratio;
    out[6] = (ratio < a.lo || ratio > a.hi) ? 1.0f : 0.0f;
}

template <int NJ>
__global__ __launch_bounds__(256) void ppo_loss_kernel(PpoArgs a) {
    static __shared__ double part[4][kPpoCols];
    loss_rows<kPpoCols>(a.B, a.iters, a.rows, a.partial, part,
                        [&](size_t b, int lane, float (&r)[kPpoCols]) { ppo_row<NJ>(a, b, lane, r); });
}

// One workgroup: the G partials -> the seven terms.  (The ratio column is added with the others and its sum is not used.)
__global__ __launch_bounds__(kA2cWidth) void ppo_terms_kernel(const double *partial, int G, int B, int M, double vc, double ec,
                                                              double ic, double mc, float *terms) {
    static __shared__ double part[kPpoCols][kA2cWidth];
    loss_sums<kPpoCols>(partial, G, part);
    if (threadIdx.x == 0) {
        const double n = (double)B, nm = (double)B * (double)M;
        const double value_loss = part[0][0] / n, action_loss = part[1][0] / n, dist_entropy = part[2][0] / n;
        const double prob_loss = part[3][0] / nm, graph_loss = part[4][0] / nm;
        terms[0] = (float)value_loss, terms[1] = (float)action_loss, terms[2] = (float)dist_entropy;
        terms[3] = (float)prob_loss, terms[4] = (float)graph_loss;
        terms[5] = (float)(vc * value_loss + action_loss - ec * dist_entropy + ic * prob_loss + mc * graph_loss);
        terms[6] = (float)(part[6][0] / n);
    }
}

// ---- normalised advantages --------------------------------------------------------------------------------------------------
// The sum of a block's kAdvWidth lane values: a binary tree, stride kAdvWidth / 2, ..., 1; the result in every lane.
__device__ __forceinline__ double adv_block_sum(double v, double *sh) {
    const int t = threadIdx.x;
    __syncthreads();            // the previous use of sh is over
    sh[t] = v;
    __syncthreads();
    for (int d = kAdvWidth / 2; d > 0; d >>= 1) {
        if (t < d) sh[t] = sh[t] + sh[t + d];
        __syncthreads();
    }
    return sh[0];
}
// The sum of the G block sums, by every block that needs it: lane t adds sums t, t + kAdvWidth, ..., then the tree.
__device__ __forceinline__ double adv_total(const double *partial, int G, double *sh) {
    double s = 0.0;
    for (int g = threadIdx.x; g < G; g += kAdvWidth) s = s + partial[g];
    return adv_block_sum(s, sh);
}

// PASS 0: partial[g] = the block's sum of raw.  PASS 1: mean from the sums of pass 0, partial2[g] = the block's sum of
// (raw - mean)^2.  PASS 2: mean and std from both, stats, adv.
template <int PASS>
__global__ __launch_bounds__(kAdvWidth) void ppo_adv_kernel(const float *returns, const float *value_preds, float *adv, double *stats,
                                                            double *partial, double *partial2, int E, int iters, int G) {
    static __shared__ double sh[kAdvWidth];
    const size_t base = (size_t)blockIdx.x * (size_t)iters * kAdvWidth + threadIdx.x;
    double mean = 0.0, sd = 0.0;
    if constexpr (PASS >= 1) mean = adv_total(partial, G, sh) / (double)E;
    if constexpr (PASS == 2) sd = sqrt(adv_total(partial2, G, sh) / (double)(E - 1));
    if constexpr (PASS < 2) {
        double s = 0.0;
        for (int i = 0; i < iters; ++i) {
            const size_t k = base + (size_t)i * kAdvWidth;
            if (k >= (size_t)E) break;
            const float raw = returns[k] - value_preds[k];
            if constexpr (PASS == 0) {
                s = s + (double)raw;
            } else {
                const double dv = (double)raw - mean;
                s = s + dv * dv;
            }
        }
        s = adv_block_sum(s, sh);
        if (threadIdx.x == 0) (PASS == 0 ? partial : partial2)[blockIdx.x] = s;
    } else {
        if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = mean, stats[1] = sd;
        const float mean_f = (float)mean, den = (float)sd + 1e-5f;
        for (int i = 0; i < iters; ++i) {
            const size_t k = base + (size_t)i * kAdvWidth;
            if (k >= (size_t)E) break;
            const float raw = returns[k] - value_preds[k];
            adv[k] = (raw - mean_f) / den;
        }
    }
}

// elements per block = kAdvWidth * iters and blocks, from E alone
void adv_shape(int E, int &iters, int &groups) {
    const long long chunks = ((long long)E + kAdvWidth - 1) / kAdvWidth;
    iters = (int)((chunks + kAdvMaxBlocks - 1) / kAdvMaxBlocks);
    groups = (int)((chunks + iters - 1) / iters);
}

// ---- row gather -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *src, int64_t stride, int64_t rows, const int64_t *idx, int B,
                                                          int len, int parts, float *dst) {
    const int lane = threadIdx.x & (kWave - 1);
    const size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const size_t b = w / (size_t)parts;
    if (b >= (size_t)B) return;
    const int k0 = (int)(w % (size_t)parts) * kGatherPart, k1 = min(len, k0 + kGatherPart);
    const int64_t r = idx[b];
    float *d = dst + b * (size_t)len;
    if (r < 0 || r >= rows) {
        for (int k = k0 + lane; k < k1; k += kWave) d[k] = __builtin_nanf("");
        return;
    }
    const float *s = src + (size_t)r * (size_t)stride;
    for (int k = k0 + lane; k < k1; k += kWave) d[k] = s[k];
}

}  // namespace

extern "C" {

size_t bpp_ppo_advantages_workspace(int32_t E) {
    if (E < 2) return 0;
    int iters, groups;
    adv_shape(E, iters, groups);
    return (size_t)groups * 2 * sizeof(double);
}

int bpp_ppo_advantages_info(int32_t E, int32_t out[3]) {
    const ArgCheck ck{"bpp_ppo_advantages_info"};
    if (E < 2) return ck.bad("E must be >= 2");
    if (!out) return ck.bad("NULL out");
    int iters, groups;
    adv_shape(E, iters, groups);
    out[0] = kAdvWidth * iters, out[1] = groups, out[2] = kAdvWidth;
    return 0;
}

int bpp_ppo_advantages(const float *returns, const float *value_preds, float *adv, double *stats, int32_t E, void *workspace,
                       void *stream) {
    const ArgCheck ck{"bpp_ppo_advantages"};
    if (E < 2) return ck.bad("E must be >= 2 (the unbiased standard deviation divides by E - 1)");
    if (!returns || !value_preds || !adv || !stats || !workspace) return ck.bad("NULL pointer");
    int iters, groups;
    adv_shape(E, iters, groups);
    double *p1 = (double *)workspace, *p2 = p1 + groups;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_adv_kernel<0>, dim3(groups), dim3(kAdvWidth), 0, st, returns, value_preds, adv, stats, p1, p2, E, iters, groups);
    int rc = launched();
    if (rc) return rc;
    hipLaunchKernelGGL(ppo_adv_kernel<1>, dim3(groups), dim3(kAdvWidth), 0, st, returns, value_preds, adv, stats, p1, p2, E, iters, groups);
    rc = launched();
    if (rc) return rc;
    hipLaunchKernelGGL(ppo_adv_kernel<2>, dim3(groups), dim3(kAdvWidth), 0, st, returns, value_preds, adv, stats, p1, p2, E, iters, groups);
    return launched();
}

int bpp_gather_rows(const float *src, int64_t src_stride, int64_t rows, const int64_t *idx, int32_t B, int32_t len, float *dst,
                    void *stream) {
    const ArgCheck ck{"bpp_gather_rows"};
    if (B < 1 || len < 1 || rows < 1) return ck.bad("B, len and rows must be >= 1");
    if (src_stride < len) return ck.bad("src_stride < len");
    if (!src || !idx || !dst) return ck.bad("NULL pointer");
    const int parts = (len + kGatherPart - 1) / kGatherPart;
    const long long groups = ((long long)B * parts + 3) / 4;
    if (groups > 0x7fffffffLL) return ck.bad("B * len too large for one launch");
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, src, src_stride, rows, idx, B, len,
                       parts, dst);
    return launched();
}

size_t bpp_ppo_loss_workspace(int32_t B, int32_t M) {
    if (B < 1 || M < 1) return 0;
    int iters, groups;
    a2c_shape(B, iters, groups);
    return (size_t)groups * kPpoCols * sizeof(double);
}

int bpp_ppo_loss_info(int32_t B, int32_t M, int32_t out[4]) {
    const ArgCheck ck{"bpp_ppo_loss_info"};
    if (B < 1 || M < 1) return ck.bad("B and M must be >= 1");
    if (!out) return ck.bad("NULL out");
    int iters, groups;
    a2c_shape(B, iters, groups);
    out[0] = 4 * iters, out[1] = groups, out[2] = a2c_regs(M) > 0, out[3] = kA2cWidth;
    return 0;
}

int bpp_ppo_loss(const float *logits, const float *values, const float *pred_mask, const int64_t *idx, const float *location_masks,
                 const int64_t *action, const float *value_preds, const float *returns, const float *old_log_probs, const float *adv,
                 double clip, double value_loss_coef, double entropy_coef, double invalid_coef, double mask_coef,
                 int32_t use_clipped_value_loss, float *grad_logits, float *grad_values, float *grad_pred_mask, float *rows,
                 float *terms, void *workspace, int32_t B, int32_t E, int32_t M, void *stream) {
    const ArgCheck ck{"bpp_ppo_loss"};
    if (B < 1 || E < 1 || M < 1) return ck.bad("B, E and M must be >= 1");
    if (!(clip >= 0.0)) return ck.bad("clip must be >= 0");
    if (!idx && B > E) return ck.bad("without idx the mini-batch is rows 0 .. B - 1 of the rollout: B > E");
    if (!logits || !values || !location_masks || !action || !value_preds || !returns || !old_log_probs || !adv || !grad_logits ||
        !grad_values || !terms || !workspace)
        return ck.bad("NULL pointer");
    if (pred_mask && !grad_pred_mask) return ck.bad("pred_mask without grad_pred_mask");
    PpoArgs a;
    a.logits = logits, a.values = values, a.pred = pred_mask, a.mask = location_masks, a.value_preds = value_preds, a.returns = returns;
    a.old = old_log_probs, a.adv = adv, a.idx = idx, a.action = action;
    a.g_logits = grad_logits, a.g_values = grad_values, a.g_pred = grad_pred_mask, a.rows = rows, a.partial = (double *)workspace;
    a.B = B, a.E = E, a.M = M, a.clipped_value = use_clipped_value_loss != 0;
    int groups;
    a2c_shape(B, a.iters, groups);
    const double n = (double)B, nm = (double)B * (double)M;
    a.lo = (float)(1.0 - clip), a.hi = (float)(1.0 + clip), a.c = (float)clip;
    a.cB = (float)(1.0 / n);
    a.c_v = (float)(value_loss_coef / n);
    a.g_ent = (float)(-entropy_coef / n);
    a.g_bad = (float)(invalid_coef / nm);
    a.c_p = (float)(2.0 * mask_coef / nm);
    const hipStream_t st = (hipStream_t)stream;
    switch (a2c_regs(M)) {
        case 1: hipLaunchKernelGGL(ppo_loss_kernel<1>, dim3(groups), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(ppo_loss_kernel<2>, dim3(groups), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL(ppo_loss_kernel<4>, dim3(groups), dim3(256), 0, st, a); break;
        case 8: hipLaunchKernelGGL(ppo_loss_kernel<8>, dim3(groups), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(ppo_loss_kernel<0>, dim3(groups), dim3(256), 0, st, a); break;
    }
    const int rc = launched();
    if (rc) return rc;
    hipLaunchKernelGGL(ppo_terms_kernel, dim3(1), dim3(kA2cWidth), 0, st, (const double *)workspace, groups, B, M, value_loss_coef,
                       entropy_coef, invalid_coef, mask_coef, terms);
    return launched();
}

}  // extern "C"
