// bpp_update.inl -- the loss of the A2C update and its gradients in one pass (include/bpp_update.h), included at the
// end of bpp_kernels.hip: the five terms of acktr/algo/acktr_pipeline.py:45-92 and d loss / d (logits, values, pred_mask).
//
// One wave per row, four rows at a time per 256-lane workgroup, as the evaluate kernels of bpp_heads.inl -- and through the same
// row body, row_stats and row_terms, built from the same expressions: the bits are theirs by construction.  What differs is how
// often memory is visited: for M <= 512 the row is a RegRow, a lane keeps its <= 8 entries of logits and location mask in
// registers together with the values the evaluate kernels compute two to four times (the two exponentials, the probability's
// h), so each input array is read once per row and each gradient array is written once.  Longer rows are a MemRow, as in
// masked_eval_*_kernel.
//
// The sums of the five per-row terms are taken in double, without atomics, in an order fixed by E alone: a workgroup owns
// `4 * iters` consecutive rows and publishes one partial, at most kA2cWidth partials exist, one final workgroup adds them.
// LossRow, pred_mask_row, loss_rows, loss_sums, a2c_shape and a2c_regs are shared with the PPO loss (bpp_ppo.inl).

namespace {

constexpr int kA2cWidth = 1024;     // partials of the row kernel at most = lanes of the final workgroup
constexpr int kA2cMaxRegs = 8;      // entries of a row a lane holds in registers: M <= 64 * 8

struct A2cArgs {
    const float *logits, *mask, *values, *returns, *pred;
    const int64_t *action;
    float *g_logits, *g_values, *g_pred, *rows;
    double *partial;
    int E, M, iters;
    float cE, g_ent, g_bad, c_v, c_p;
};

// Row e through row_stats and row_terms (bpp_heads.inl): NJ > 0 entries per lane in registers (M <= 64 * NJ), NJ = 0 a row of
// any length walked in memory.  out = {adv * adv, -(adv * logp), ent, bad, sq}, in every lane.
template <int NJ>
using LossRow = std::conditional_t<(NJ > 0), RegRow<(NJ > 0) ? NJ : 1>, MemRow>;

// The mask-prediction term of a row (shared with bpp_ppo.inl): sq = sum_k (pred[k] - mask[k])^2 in every lane, and
// g_pred[k] = c_p (pred[k] - mask[k]).  pred and g_pred point at the row.
template <int NJ>
__device__ __forceinline__ float pred_mask_row(const LossRow<NJ> &row, const float *pred, float *g_pred, float c_p) {
    constexpr bool kRegs = NJ > 0;
    float s = 0.0f;
    float pv[kRegs ? NJ : 1];       // the register form: every load of the row is issued before any arithmetic
    if constexpr (kRegs) row.each([&](int j, int k) { pv[j] = pred[k]; });
    row.each([&](int j, int k) {
        const float d = (kRegs ? pv[j] : pred[k]) - row.m(j, k);
        s += d * d;
        g_pred[k] = c_p * d;
    });
    return wave_sum(s);
}

template <int NJ>
__device__ __forceinline__ void a2c_row(const A2cArgs &a, size_t e, int lane, float (&out)[5]) {
    const int M = a.M;
    const size_t off = e * (size_t)M;
    const float *x = a.logits + off, *m = a.mask + off;
    LossRow<NJ> row(x, m, M, lane);
    const float s = a.pred ? pred_mask_row<NJ>(row, a.pred + off, a.g_pred + off, a.c_p) : 0.0f;
    const float adv = a.returns[e] - a.values[e];
    const HeadGrad w{a.action[e], -(adv * a.cE), a.g_ent, a.g_bad};
    float h, b;
    const RowStats r = row_stats(row);
    row_terms<true, true>(row, r, w, a.g_logits + off, h, b);
    const float logp = action_logp(x, m, M, w.act, r);
    if (lane == 0) a.g_values[e] = a.c_v * adv;
    out[0] = adv * adv, out[1] = -(adv * logp), out[2] = h, out[3] = b, out[4] = s;
}

// The sums of NC per-row terms, shared with bpp_ppo.inl.  loss_rows: a 256-lane workgroup owns rows [blockIdx.x 4 iters, + 4 iters) of
// n, wave w takes rows w, w + 4, ...; fn(row, lane, out) computes a row's NC terms in every lane; they are added in double, stored
// to rows[row][0 .. NC) when asked for, and the workgroup publishes ((w0 + w1) + w2) + w3 as partial[blockIdx.x][0 .. NC).
template <int NC, typename RowFn>
__device__ __forceinline__ void loss_rows(int n, int iters, float *rows, double *partial, double (*part)[NC], RowFn fn) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const size_t e0 = (size_t)blockIdx.x * 4u * (size_t)iters;
    double acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.0;
    for (int i = 0; i < iters; ++i) {
        const size_t e = e0 + 4u * (size_t)i + (size_t)wave;
        if (e >= (size_t)n) break;       // a whole wave: its later rows lie further out still
        float r[NC];
        fn(e, lane, r);
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] = acc[j] + (double)r[j];
        if (lane == 0 && rows) {
#pragma unroll
            for (int j = 0; j < NC; ++j) rows[e * NC + j] = r[j];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NC; ++j) part[wave][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        const int j = threadIdx.x;
        partial[(size_t)blockIdx.x * NC + j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
    }
}

// loss_sums: ONE workgroup of kA2cWidth lanes adds the G partials of loss_rows; lane t takes partials t, t + kA2cWidth, ..., a
// binary tree (stride kA2cWidth / 2, ..., 1) adds the lanes.  Afterwards part[j][0] is the sum of column j (valid in lane 0).
template <int NC>
__device__ __forceinline__ void loss_sums(const double *partial, int G, double (*part)[kA2cWidth]) {
    const int t = threadIdx.x;
    double s[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) s[j] = 0.0;
    for (int gi = t; gi < G; gi += kA2cWidth) {
#pragma unroll
        for (int j = 0; j < NC; ++j) s[j] = s[j] + partial[(size_t)gi * NC + j];
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) part[j][t] = s[j];
    __syncthreads();
    for (int d = kA2cWidth / 2; d > 0; d >>= 1) {
        if (t < d) {
#pragma unroll
            for (int j = 0; j < NC; ++j) part[j][t] = part[j][t] + part[j][t + d];
        }
        __syncthreads();
    }
}

template <int NJ>
__global__ __launch_bounds__(256) void a2c_loss_kernel(A2cArgs a) {
    static __shared__ double part[4][5];
    loss_rows<5>(a.E, a.iters, a.rows, a.partial, part, [&](size_t e, int lane, float (&r)[5]) { a2c_row<NJ>(a, e, lane, r); });
}

// One workgroup: the G partials -> the six terms.
__global__ __launch_bounds__(kA2cWidth) void a2c_terms_kernel(const double *partial, int G, int E, int M, double vc, double ec,
                                                              double ic, double mc, float *terms) {
    static __shared__ double part[5][kA2cWidth];
    loss_sums<5>(partial, G, part);
    if (threadIdx.x == 0) {
        const double n = (double)E, nm = (double)E * (double)M;
        const double value_loss = part[0][0] / n, action_loss = part[1][0] / n, dist_entropy = part[2][0] / n;
        const double prob_loss = part[3][0] / nm, graph_loss = part[4][0] / nm;
        terms[0] = (float)value_loss, terms[1] = (float)action_loss, terms[2] = (float)dist_entropy;
        terms[3] = (float)prob_loss, terms[4] = (float)graph_loss;
        terms[5] = (float)(vc * value_loss + action_loss + ic * prob_loss - ec * dist_entropy + mc * graph_loss);
    }
}

// rows per workgroup = 4 * iters and workgroups, from E alone
void a2c_shape(int E, int &iters, int &groups) {
    const long long quads = ((long long)E + 3) / 4;
    iters = (int)((quads + kA2cWidth - 1) / kA2cWidth);
    groups = (int)((quads + iters - 1) / iters);
}

int a2c_regs(int M) { return M <= 64 ? 1 : M <= 128 ? 2 : M <= 256 ? 4 : M <= kWave * kA2cMaxRegs ? 8 : 0; }

}  // namespace

extern "C" {

size_t bpp_a2c_loss_workspace(int32_t E, int32_t M) {
    if (E < 1 || M < 1) return 0;
    int iters, groups;
    a2c_shape(E, iters, groups);
    return (size_t)groups * 5 * sizeof(double);
}

int bpp_a2c_loss_info(int32_t E, int32_t M, int32_t out[4]) {
    const ArgCheck ck{"bpp_a2c_loss_info"};
    if (E < 1 || M < 1) return ck.bad("E and M must be >= 1");
    if (!out) return ck.bad("NULL out");
    int iters, groups;
    a2c_shape(E, iters, groups);
    out[0] = 4 * iters, out[1] = groups, out[2] = a2c_regs(M) > 0, out[3] = kA2cWidth;
    return 0;
}

int bpp_a2c_loss(const float *logits, const float *location_masks, const int64_t *action, const float *values, const float *returns,
                 const float *pred_mask, double value_loss_coef, double entropy_coef, double invalid_coef, double mask_coef,
                 float *grad_logits, float *grad_values, float *grad_pred_mask, float *rows, float *terms, void *workspace, int32_t E,
                 int32_t M, void *stream) {
    const ArgCheck ck{"bpp_a2c_loss"};
    if (E < 1 || M < 1) return ck.bad("E and M must be >= 1");
    if (!logits || !location_masks || !action || !values || !returns || !grad_logits || !grad_values || !terms || !workspace)
        return ck.bad("NULL pointer");
    if (pred_mask && !grad_pred_mask) return ck.bad("pred_mask without grad_pred_mask");
    A2cArgs a;
    a.logits = logits, a.mask = location_masks, a.values = values, a.returns = returns, a.pred = pred_mask, a.action = action;
    a.g_logits = grad_logits, a.g_values = grad_values, a.g_pred = grad_pred_mask, a.rows = rows, a.partial = (double *)workspace;
    a.E = E, a.M = M;
    int groups;
    a2c_shape(E, a.iters, groups);
    const double n = (double)E, nm = (double)E * (double)M;
    a.cE = (float)(1.0 / n);
    a.g_ent = (float)(-entropy_coef / n);
    a.g_bad = (float)(invalid_coef / nm);
    a.c_v = (float)(-2.0 * value_loss_coef / n);
    a.c_p = (float)(2.0 * mask_coef / nm);
    const hipStream_t st = (hipStream_t)stream;
    switch (a2c_regs(M)) {
        case 1: hipLaunchKernelGGL(a2c_loss_kernel<1>, dim3(groups), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(a2c_loss_kernel<2>, dim3(groups), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL(a2c_loss_kernel<4>, dim3(groups), dim3(256), 0, st, a); break;
        case 8: hipLaunchKernelGGL(a2c_loss_kernel<8>, dim3(groups), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(a2c_loss_kernel<0>, dim3(groups), dim3(256), 0, st, a); break;
    }
    const int rc = launched();
    if (rc) return rc;
    hipLaunchKernelGGL(a2c_terms_kernel, dim3(1), dim3(kA2cWidth), 0, st, (const double *)workspace, groups, E, M, value_loss_coef,
                       entropy_coef, invalid_coef, mask_coef, terms);
    return launched();
}

}  // extern "C"
