// bpp_returns.inl -- returns of a rollout that lives in [rows][N] slabs (include/bpp_rollout.h), included at the end of
// bpp_kernels.hip: the four variants of the reference's RolloutStorage.compute_returns (acktr/storage.py:72-111) as one launch.
//
// The recurrence runs backwards in t and never looks at another bin: a lane owns V adjacent bins (V = 4: 16-byte accesses; V = 1: any
// N, any alignment) and keeps the running value in registers.  Only the carried value is sequential -- the loads of rewards, value
// predictions and masks do not depend on it, so a lane fetches kReturnsRows time steps at once (independent loads, one memory latency
// per kReturnsRows rows instead of one per row) and then runs the arithmetic over them.  No LDS, no atomics, no word shared between lanes.

namespace {

// ONE step of the recurrence of ONE bin, float32 and unfused (-ffp-contract=off), in the operation order of the reference's tensor
// expressions.  `carry`: gae (use_gae) or returns[t + 1]; v_next = value_preds[t + 1] (only read under use_gae); m, bad = row t + 1.
// Returns returns[t].  The device kernels and bpp_compute_returns_host all run this text.
__host__ __device__ inline float returns_step(int use_gae, int proper, float g, float gl, float r, float v, float v_next, float m,
                                              float bad, float &carry) {
    if (use_gae) {
        const float delta = (r + (g * v_next) * m) - v;
        float gae = delta + (gl * m) * carry;
        if (proper) gae = gae * bad;
        carry = gae;
        return gae + v;
    }
    float ret = ((carry * g) * m) + r;
    if (proper) ret = ret * bad + (1.0f - bad) * v;
    carry = ret;
    return ret;
}

struct ReturnsArgs {
    const float *rewards, *next_value, *bad_masks;
    const uint8_t *done;
    float *value_preds, *masks, *returns, *advantages;
    int T, N, use_gae, proper;
    float g, gl;
};

constexpr int kReturnsRows = 8;       // time steps a lane has in flight
constexpr int kReturnsVecLanes = 64;  // V = 4: one wave = 256 bins per workgroup, so that 65 536 bins make 256 workgroups -- one per CU
constexpr int kReturnsLanes = 256;    // V = 1

template <int V>
__device__ __forceinline__ void ret_get(const float *p, float (&a)[V]) {
    if constexpr (V == 4) {
        const float4 q = *(const float4 *)p;
        a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
    } else {
        a[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void ret_put(float *p, const float (&a)[V]) {
    if constexpr (V == 4) {
        *(float4 *)p = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        *p = a[0];
    }
}

// done bytes of V adjacent bins -> the float mask of the reference (main.py:172: 0.0 where the episode ended, else 1.0)
template <int V>
__device__ __forceinline__ void ret_get_done(const uint8_t *p, float (&m)[V]) {
    if constexpr (V == 4) {
        const uint32_t w = *(const uint32_t *)p;
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ((w >> (8 * k)) & 255u) ? 0.0f : 1.0f;
    } else {
        m[0] = *p ? 0.0f : 1.0f;
    }
}

template <int V>
__global__ __launch_bounds__(V == 4 ? kReturnsVecLanes : kReturnsLanes) void returns_kernel(ReturnsArgs a) {
    const size_t N = (size_t)a.N;
    const size_t n0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V;     // this lane's first bin
    if (n0 >= N) return;                                                       // (V = 4 runs with N % 4 == 0 only: no partial lane)
    const int T = a.T;
    const bool need_v = a.use_gae || a.proper || a.advantages;                 // the plain variant without advantages never reads value_preds
    float carry[V], v_next[V];
    ret_get<V>(a.next_value + n0, v_next);
    if (a.use_gae) {
        ret_put<V>(a.value_preds + (size_t)T * N + n0, v_next);          // storage.py:80,98
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = 0.0f;
    } else {
        ret_put<V>(a.returns + (size_t)T * N + n0, v_next);              // storage.py:91,108
#pragma unroll
        for (int k = 0; k < V; ++k) carry[k] = v_next[k];
    }
    for (int t0 = T; t0 > 0; t0 -= kReturnsRows) {                             // rows t0 - 1 .. t0 - cnt of this chunk
        const int cnt = t0 < kReturnsRows ? t0 : kReturnsRows;
        float r[kReturnsRows][V], v[kReturnsRows][V], m[kReturnsRows][V], bad[kReturnsRows][V];
#pragma unroll
        for (int u = 0; u < kReturnsRows; ++u) {
            if (u < cnt) {
                const size_t t = (size_t)(t0 - 1 - u);
                ret_get<V>(a.rewards + t * N + n0, r[u]);
                if (need_v) {
                    ret_get<V>(a.value_preds + t * N + n0, v[u]);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) v[u][k] = 0.0f;
                }
                if (a.done) ret_get_done<V>(a.done + t * N + n0, m[u]);
                else ret_get<V>(a.masks + (t + 1) * N + n0, m[u]);
                if (a.bad_masks) {
                    ret_get<V>(a.bad_masks + (t + 1) * N + n0, bad[u]);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) bad[u][k] = 1.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kReturnsRows; ++u) {
            if (u < cnt) {
                const size_t t = (size_t)(t0 - 1 - u);
                float ret[V];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    ret[k] = returns_step(a.use_gae, a.proper, a.g, a.gl, r[u][k], v[u][k], v_next[k], m[u][k], bad[u][k], carry[k]);
                    v_next[k] = v[u][k];
                }
                ret_put<V>(a.returns + t * N + n0, ret);
                if (a.done && a.masks) ret_put<V>(a.masks + (t + 1) * N + n0, m[u]);
                if (a.advantages) {
                    float adv[V];
#pragma unroll
                    for (int k = 0; k < V; ++k) adv[k] = ret[k] - v[u][k];
                    ret_put<V>(a.advantages + t * N + n0, adv);
                }
            }
        }
    }
}

int returns_check(const ReturnsArgs &a, const ArgCheck &ck) {
    if (a.T < 1 || a.N < 1) return ck.bad("T and N must be >= 1");
    if (!a.rewards || !a.value_preds || !a.next_value || !a.returns) return ck.bad("NULL pointer");
    if (!a.done && !a.masks) return ck.bad("give done or masks");
    return 0;
}

ReturnsArgs returns_args(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                         const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                         int32_t proper, double gamma, double gae_lambda) {
    ReturnsArgs a;
    a.rewards = rewards, a.next_value = next_value, a.bad_masks = bad_masks, a.done = done;
    a.value_preds = value_preds, a.masks = masks, a.returns = returns, a.advantages = advantages;
    a.T = T, a.N = N, a.use_gae = use_gae != 0, a.proper = proper != 0;
    a.g = (float)gamma;
    a.gl = (float)(gamma * gae_lambda);      // Python multiplies the two floats first, torch rounds the product to float32
    return a;
}

// The form a call takes: 4 bins per lane (16-byte accesses) when every row of every array starts 16-byte aligned -- exactly when the
// array does and N is a multiple of 4 (done rows: 4-byte) --, else one bin per lane.  NULL pointers are aligned.
int returns_bins_per_lane(const ReturnsArgs &a) {
    const uintptr_t f32 = (uintptr_t)a.rewards | (uintptr_t)a.value_preds | (uintptr_t)a.next_value | (uintptr_t)a.masks |
                          (uintptr_t)a.bad_masks | (uintptr_t)a.returns | (uintptr_t)a.advantages;
    return (a.N % 4 == 0 && (f32 & 15u) == 0 && ((uintptr_t)a.done & 3u) == 0) ? 4 : 1;
}

unsigned returns_workgroups(const ReturnsArgs &a, int V) {
    const unsigned lanes = V == 4 ? (unsigned)(a.N / 4) : (unsigned)a.N, per = V == 4 ? kReturnsVecLanes : kReturnsLanes;
    return (lanes + per - 1) / per;
}

}  // namespace

extern "C" {

int bpp_compute_returns(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                        const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                        int32_t use_proper_time_limits, double gamma, double gae_lambda, void *stream) {
    const ReturnsArgs a = returns_args(rewards, value_preds, next_value, done, masks, bad_masks, returns, advantages, T, N, use_gae,
                                       use_proper_time_limits, gamma, gae_lambda);
    const int rc = returns_check(a, ArgCheck{"bpp_compute_returns"});
    if (rc) return rc;
    if (returns_bins_per_lane(a) == 4) {
        hipLaunchKernelGGL(returns_kernel<4>, dim3(returns_workgroups(a, 4)), dim3(kReturnsVecLanes), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(returns_kernel<1>, dim3(returns_workgroups(a, 1)), dim3(kReturnsLanes), 0, (hipStream_t)stream, a);
    }
    return launched();
}

int bpp_compute_returns_info(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                             const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                             int32_t use_proper_time_limits, double gamma, double gae_lambda, int32_t out[3]) {
    const ReturnsArgs a = returns_args(rewards, value_preds, next_value, done, masks, bad_masks, returns, advantages, T, N, use_gae,
                                       use_proper_time_limits, gamma, gae_lambda);
    const ArgCheck ck{"bpp_compute_returns_info"};
    const int rc = returns_check(a, ck);
    if (rc) return rc;
    if (!out) return ck.bad("NULL out");
    const int V = returns_bins_per_lane(a);
    out[0] = V, out[1] = V == 4 ? kReturnsVecLanes : kReturnsLanes, out[2] = (int32_t)returns_workgroups(a, V);
    return 0;
}

int bpp_compute_returns_host(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                             const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                             int32_t use_proper_time_limits, double gamma, double gae_lambda) {
    const ReturnsArgs a = returns_args(rewards, value_preds, next_value, done, masks, bad_masks, returns, advantages, T, N, use_gae,
                                       use_proper_time_limits, gamma, gae_lambda);
    const int rc = returns_check(a, ArgCheck{"bpp_compute_returns_host"});
    if (rc) return rc;
    const size_t n_bins = (size_t)N;
    for (size_t n = 0; n < n_bins; ++n) {
        float v_next = next_value[n], carry;
        if (a.use_gae) {
            value_preds[(size_t)T * n_bins + n] = v_next;
            carry = 0.0f;
        } else {
            returns[(size_t)T * n_bins + n] = v_next;
            carry = v_next;
        }
        for (int t = T - 1; t >= 0; --t) {
            const size_t i = (size_t)t * n_bins + n, i1 = i + n_bins;
            const float m = done ? (done[i] ? 0.0f : 1.0f) : masks[i1];
            const float bad = bad_masks ? bad_masks[i1] : 1.0f;
            const float v = value_preds[i];
            const float ret = returns_step(a.use_gae, a.proper, a.g, a.gl, rewards[i], v, v_next, m, bad, carry);
            v_next = v;
            returns[i] = ret;
            if (done && masks) masks[i1] = m;
            if (advantages) advantages[i] = ret - v;
        }
    }
    return 0;
}

}  // extern "C"
