// bpp_heads.inl -- the action-selection kernels, included by bpp_kernels.hip inside its anonymous namespace after bpp_wave.inl (the
// wave primitives): the uniform-feasible samplers of the benchmark policy (bpp_sample_feasible), the masked categorical head of
// the policy (bpp_masked_act / bpp_masked_act_counter; acktr/distributions.py:71-84) and its training half (bpp_masked_evaluate
// / _backward; acktr/model.py:90-96).  The head's float32 expressions are stated once, right below, and the training half's row
// body once (row_stats, row_terms): bpp_a2c_loss (bpp_update.inl) is a third instantiation of it.  Host entry points: bpp_kernels.hip.

// ---- the masked head's expressions (acktr/distributions.py:71-101), float32, built with -ffp-contract=off ------------------
//   lx = softmax(x - 14 (1 - mask)) + 1e-5,   p = lx / sum(lx),   log(clamp(p)) with torch's probs_to_logits clamp
// Whoever needs one of them calls it from here, so operation order and associativity are the same everywhere.
constexpr float kProbEps = 1.1920928955078125e-7f;   // torch.finfo(float32).eps, probs_to_logits clamp
constexpr float kProbFloor = 1e-5f;                  // distributions.py:79-80
__device__ __forceinline__ float masked_logit(float x, float m) { return x - (1.0f - m) * 14.0f; }   // distributions.py:76-79
__device__ __forceinline__ float clamp_log(float p) { return logf(fminf(fmaxf(p, kProbEps), 1.0f - kProbEps)); }
struct RowStats {
    float mq, ma, sq, sa, tot;   // maxima and denominators of the masked / plain softmax, sum of lx
    __device__ __forceinline__ float eq(float x, float m) const { return expf(masked_logit(x, m) - mq); }
    __device__ __forceinline__ float ea(float x) const { return expf(x - ma); }
    __device__ __forceinline__ float q(float x, float m) const { return eq(x, m) / sq; }      // masked softmax
    __device__ __forceinline__ float av(float x) const { return ea(x) / sa; }                 // plain softmax
    __device__ __forceinline__ float p(float q) const { return (q + kProbFloor) / tot; }
};
// d loss / d p_k given lg = clamp_log(p): the entropy term, and the log-probability term on the entry that is the action taken
// (the clamp's derivative is 0 outside)
__device__ __forceinline__ float head_hk(bool taken, float p, float lg, float gl, float ge) {
    const bool inside = p > kProbEps && p < 1.0f - kProbEps;
    const float pc = fminf(fmaxf(p, kProbEps), 1.0f - kProbEps);
    float h = -ge * (lg + (inside ? p / pc : 0.0f));
    if (taken) h += inside ? gl / pc : 0.0f;
    return h;
}
// log-probability of action a of row (x, m); an action outside [0, M) is no entry of the row: log(clamp(eps))
__device__ __forceinline__ float action_logp(const float *x, const float *m, int M, int64_t a, const RowStats &r) {
    return clamp_log((a >= 0 && a < M) ? r.p(r.q(x[a], m[a])) : kProbEps);
}

// Sub-groups of 16 lanes per bin (4 bins per wave): each lane owns `per` consecutive float4 quads of
// the bin's mask row (16-byte loads), an inclusive scan inside the 16-lane row locates the pick-th set
// entry in index order.  pick = (hash >> 32) * count >> 32.
template <int PER>
__global__ __launch_bounds__(256) void sample_kernel(const float *mask, int64_t *actions, int E, int M,
                                                     int64_t env_id_base, uint64_t seed, uint64_t step) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = tid >> 4, sl = threadIdx.x & 15;
    const bool active = e < E;
    const float4 *m = (const float4 *)(mask + (size_t)(active ? e : 0) * M);
    const int nq = M >> 2;
    float4 q[PER];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int qi = sl * PER + k;
        q[k] = (active && qi < nq) ? m[qi] : make_float4(0.f, 0.f, 0.f, 0.f);
        cnt += (q[k].x != 0.f) + (q[k].y != 0.f) + (q[k].z != 0.f) + (q[k].w != 0.f);
    }
    const int incl = wave_scan_incl<16>(cnt, sl);
    const int total = __shfl(incl, 15, 16);
    if (!active) return;
    if (total == 0) {
        if (sl == 0) actions[e] = 0;
        return;
    }
    int pick = (int)__umulhi(mix32(mix32_base(seed, step), (uint32_t)(env_id_base + e)), (uint32_t)total);
    const int excl = incl - cnt;
    if (pick >= excl && pick < incl) {
        pick -= excl;
        int found = 0, c = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const float v[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (v[t] != 0.f) {
                    if (c == pick) found = (sl * PER + k) * 4 + t;
                    ++c;
                }
        }
        actions[e] = found;
    }
}

// Masked categorical action selection (include/bpp_abi.h: bpp_masked_act; acktr/distributions.py:71-84,
// acktr/model.py:56-68).  16 lanes per bin = one DPP row, PER float4 quads of logits and mask per lane (lane sl owns quads
// sl, sl + 16, ...: every load instruction of a row is one contiguous 256-byte segment).  Round 6: the kernel is VALU-issue
// bound, not memory bound -- 65 536 rows of M = 100 are 16 waves per SIMD, and round 1's 680 instructions per wave
// (38 ds_bpermute shuffles with their address arithmetic, two IEEE divisions, logf, per-element range predicates) were 16.2 us
// for 53 MB.  Now: row maximum, softmax denominator, probability total, the inclusive scan of the CDF and the index
// reductions run on the DPP data path (row_ror / row_shr: one VALU instruction each, no LDS), the exponential, the
// reciprocals and the logarithm are the hardware's (v_exp_f32 / v_rcp_f32 / v_log_f32, ~1 ulp: inside the 5e-6
// log-probability budget the kernel is held to against a float64 reference of the formula, tests/test_policy_head_f64.py),
// a quad past the end of the row is a -inf logit instead of a predicate per element, the sampled entry is found by
// COUNTING the cumulative sums below the target, and the lane that owns the chosen entry writes the outputs (no broadcast
// of its probability): ~340 instructions per wave.
// The dpp_* / row16_* helpers: bpp_wave.inl.
template <int PER, bool DET>
__global__ __launch_bounds__(256) void masked_act_kernel(const float *logits, const float *mask, int64_t *action,
                                                         float *log_prob, int E, int M, int64_t env_id_base,
                                                         uint64_t seed, uint64_t step, const uint64_t *seed_step) {
    if (seed_step != nullptr) seed = seed_step[0], step = seed_step[1];   // bpp_masked_act_counter: (seed, step) live in device memory
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = tid >> 4, sl = threadIdx.x & 15;
    const bool active = e < E;
    const size_t row = (size_t)(active ? e : 0) * M;
    const float4 *xq = (const float4 *)(logits + row), *mq = (const float4 *)(mask + row);
    const int nq = M >> 2;
    float4 xv[PER], mv[PER];
    bool in[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {      // every load of both operands is issued before any arithmetic
        const int qi = sl + 16 * k;
        in[k] = qi < nq;
        // a quad past the end of the row behaves like four entries that can never be chosen: logit -inf (probability 0 before
        // the floor), and the 1e-5 floor itself is switched off for it below
        xv[k] = in[k] ? xq[qi] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        mv[k] = in[k] ? mq[qi] : make_float4(1.f, 1.f, 1.f, 1.f);
    }
    float z[PER][4];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        z[k][0] = masked_logit(xv[k].x, mv[k].x);
        z[k][1] = masked_logit(xv[k].y, mv[k].y);
        z[k][2] = masked_logit(xv[k].z, mv[k].z);
        z[k][3] = masked_logit(xv[k].w, mv[k].w);
        mx = fmaxf(fmaxf(mx, fmaxf(z[k][0], z[k][1])), fmaxf(z[k][2], z[k][3]));
    }
    mx = row16_max(mx);
    float part = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // exp(z - mx); exp2(-inf) = 0.  The maximum is subtracted BEFORE the scaling: z * log2e - mx * log2e rounds
            // mx * log2e on its own, an error of ~1 ulp of 1.44 |mx| that does not cancel, so logits offset by a constant C
            // (a drifting bias) moved the log-probabilities by up to 7e-5 at |C| = 1000.  z - mx is exact for every entry
            // within a factor of 2 of the maximum, and otherwise rounds relative to the difference itself, the only thing
            // the softmax depends on (tests/test_policy_head_f64.py, shifted family)
            z[k][t] = __builtin_amdgcn_exp2f((z[k][t] - mx) * 1.44269504088896340736f);
            part += z[k][t];
        }
    const float inv_sum = __builtin_amdgcn_rcpf(row16_sum(part));
    float qtot[PER];
    float lane_tot = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const float floor_k = in[k] ? 1e-5f : 0.0f;       // distributions.py:79-80
        qtot[k] = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            z[k][t] = z[k][t] * inv_sum + floor_k;
            qtot[k] += z[k][t];
        }
        lane_tot += qtot[k];
    }
    const float tot = row16_sum(lane_tot);
    int a;
    if constexpr (DET) {     // dist.mode(): first index of the maximum
        float best = -1.0f;
        int best_i = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (z[k][t] > best) {
                    best = z[k][t];
                    best_i = (sl + 16 * k) * 4 + t;
                }
        const float rb = row16_max(best);
        a = row16_min(best == rb ? best_i : 0x7fffffff);
    } else {
        // inverse CDF at u * total, entries in index order (quad-row k, then lane): the chosen entry is the first one whose
        // inclusive cumulative sum exceeds the target = the NUMBER of entries whose cumulative sum does not (the sums of a
        // lane grow with the index; the handful of cases where float32 rounding makes a lane's start fall an ulp below its
        // predecessor's end move a draw by one entry whose cumulative sum equals the target to ~1e-7 -- inside the CDF
        // tolerance the kernel is held to)
        const float u = (float)(mix32(mix32_base(seed, step), (uint32_t)(env_id_base + (active ? e : 0))) >> 8) * (1.0f / 16777216.0f);
        const float target = u * tot;
        float base = 0.0f;
        int below = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const float incl = row16_scan(qtot[k]);
            float c = base + incl - qtot[k];
            int bk = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                c += z[k][t];
                bk += c <= target ? 1 : 0;
            }
            below += in[k] ? bk : 0;
            if (k + 1 < PER) base += row16_sum(qtot[k]);
        }
        a = min(row16_isum(below), M - 1);          // (every sum <= target: rounding at u ~ 1 -> last entry)
    }
    // the lane that owns entry `a` holds its probability: it writes both outputs
    const int aq = a >> 2;
    if (active && (aq & 15) == sl) {
        float pa = 0.0f;
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if ((aq >> 4) == k) {
                const int t = a & 3;
                pa = t == 0 ? z[k][0] : (t == 1 ? z[k][1] : (t == 2 ? z[k][2] : z[k][3]));
            }
        action[e] = a;
        if (log_prob) {
            const float eps = 1.1920928955078125e-7f;  // torch clamp_probs: finfo(float32).eps
            log_prob[e] = __logf(fminf(fmaxf(pa * __builtin_amdgcn_rcpf(tot), eps), 1.0f - eps));
        }
    }
}

// Same selection for rows the 16-lane kernel cannot take (M not a multiple of 4, or M > 512 such as the
// 20x20 bin with rotation, M = 800): one wave per bin, entry k lives in lane k % 64, chunk k / 64; the CDF
// walks the chunks in order with an inclusive wave scan per chunk.
__global__ __launch_bounds__(256) void masked_act_kernel_generic(const float *logits, const float *mask, int64_t *action,
                                                                 float *log_prob, int E, int M, int64_t env_id_base,
                                                                 uint64_t seed, uint64_t step, int deterministic, const uint64_t *seed_step) {
    if (seed_step != nullptr) seed = seed_step[0], step = seed_step[1];
    const int lane = threadIdx.x & (kWave - 1);
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;  // whole waves leave; no block-level synchronisation below
    const float *x = logits + (size_t)e * M, *m = mask + (size_t)e * M;
    const int nchunk = (M + kWave - 1) / kWave;
    float mx = -INFINITY;
    for (int k = lane; k < M; k += kWave) mx = fmaxf(mx, masked_logit(x[k], m[k]));
    mx = wave_max(mx);
    float part = 0.0f;
    for (int k = lane; k < M; k += kWave) part += expf(masked_logit(x[k], m[k]) - mx);
    const float sum = wave_sum(part);
    const auto lx = [&](int k) { return expf(masked_logit(x[k], m[k]) - mx) / sum + kProbFloor; };
    float lane_tot = 0.0f, best = -1.0f;
    int best_i = 0;
    for (int k = lane; k < M; k += kWave) {
        const float pk = lx(k);
        lane_tot += pk;
        if (pk > best) {
            best = pk;
            best_i = k;
        }
    }
    const float tot = wave_sum(lane_tot);
    int a;
    float pa;
    if (deterministic) {  // dist.mode(): first index of the maximum
        wave_argmax(best, best_i, false);
        a = best_i;
        pa = best;
    } else {
        const float u = (float)(mix32(mix32_base(seed, step), (uint32_t)(env_id_base + e)) >> 8) * (1.0f / 16777216.0f);
        const float target = u * tot;
        float base = 0.0f, pm = 0.0f;
        int cand = 0x7fffffff;
        for (int c = 0; c < nchunk; ++c) {  // wave-uniform trip count
            const int k = c * kWave + lane;
            const float pk = k < M ? lx(k) : 0.0f;
            const float incl = wave_scan_incl(pk, lane);
            if (cand == 0x7fffffff && k < M && base + incl > target) {
                cand = k;
                pm = pk;
            }
            base += __shfl(incl, kWave - 1, kWave);
        }
        wave_min_keyed(cand, pm);
        if (cand == 0x7fffffff) {  // rounding at u ~ 1: the last entry
            cand = M - 1;
            pm = lx(M - 1);
        }
        a = cand;
        pa = pm;
    }
    if (lane == 0) {
        action[e] = a;
        if (log_prob) log_prob[e] = clamp_log(pa / tot);
    }
}

// Training half of the masked policy head (acktr/distributions.py:71-101 as used by Policy.evaluate_actions,
// acktr/model.py:90-96): for the actions taken, one wave per bin computes
//   logp  = log(clamp(p[a]))            p = lx / sum(lx), lx = softmax(x - 14 (1 - mask)) + 1e-5   (dist.log_probs)
//   ent   = -sum_k p_k log(clamp(p_k))                                                           (dist.entropy())
//   bad   = sum_k softmax(x)_k (1 - mask_k)                                                      (row sum of `bx`)
// and the gradient of  gl * logp + ge * ent + gb * bad  with respect to the logits.
//
// A lane's view of one row, in two forms.  Entry k lives in lane k % 64; each(f) calls f(j, k) for the lane's entries
// k = lane + 64 j < M in ascending k.  The row body computes the per-entry values (the two exponentials, then q and av, then h) in
// passes; put_*() hands each to the row where it is first computed and the getters give it to the later passes.  MemRow keeps
// nothing and computes it again from x and m -- the same expression, so the same bits; RegRow<NJ> (M <= 64 NJ) keeps all of
// them in registers and has issued every load of the row before any arithmetic.
struct HeadGrad {
    int64_t act;        // the action taken
    float gl, ge, gb;   // weights of logp, ent and bad in the loss
};
struct MemRow {
    const float *xs, *ms;
    int M, lane;
    __device__ __forceinline__ MemRow(const float *x, const float *m, int M_, int lane_) : xs(x), ms(m), M(M_), lane(lane_) {}
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        for (int k = lane; k < M; k += kWave) f(0, k);
    }
    __device__ __forceinline__ float x(int, int k) const { return xs[k]; }
    __device__ __forceinline__ float m(int, int k) const { return ms[k]; }
    __device__ __forceinline__ float eq(int, int k, const RowStats &r) const { return r.eq(xs[k], ms[k]); }
    __device__ __forceinline__ float ea(int, int k, const RowStats &r) const { return r.ea(xs[k]); }
    __device__ __forceinline__ float q(int, int k, const RowStats &r) const { return r.q(xs[k], ms[k]); }
    __device__ __forceinline__ float av(int, int k, const RowStats &r) const { return r.av(xs[k]); }
    __device__ __forceinline__ float h(int, int k, const RowStats &r, const HeadGrad &w) const {
        const float p = r.p(r.q(xs[k], ms[k]));
        return head_hk(k == w.act, p, clamp_log(p), w.gl, w.ge);
    }
    __device__ __forceinline__ void put_e(int, float, float) const {}
    __device__ __forceinline__ void put_q(int, float) const {}
    __device__ __forceinline__ void put_av(int, float) const {}
    __device__ __forceinline__ void put_h(int, float) const {}
};
template <int NJ>
struct RegRow {
    float xv[NJ], mv[NJ], qv[NJ], avv[NJ], hv[NJ];   // logit, mask; masked exponential -> q; plain exponential -> av; h
    int M, lane;
    __device__ __forceinline__ RegRow(const float *x, const float *m, int M_, int lane_) : M(M_), lane(lane_) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = lane + kWave * j;
            const bool ok = k < M;
            xv[j] = ok ? x[k] : 0.0f;
            mv[j] = ok ? m[k] : 0.0f;
        }
    }
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + kWave * j < M) f(j, lane + kWave * j);
    }
    __device__ __forceinline__ float x(int j, int) const { return xv[j]; }
    __device__ __forceinline__ float m(int j, int) const { return mv[j]; }
    // Order contract: a slot holds a pass's value until the next pass overwrites it.  qv[j] is the masked exponential from
    // put_e until put_q and q from then on; avv[j] is the plain exponential from put_e until put_av and av from then on.  So
    // eq() / ea() are valid only before, q() / av() only after the matching put: the order row_stats and row_terms keep.
    __device__ __forceinline__ float eq(int j, int, const RowStats &) const { return qv[j]; }     // before put_q
    __device__ __forceinline__ float ea(int j, int, const RowStats &) const { return avv[j]; }    // before put_av
    __device__ __forceinline__ float q(int j, int, const RowStats &) const { return qv[j]; }      // after put_q
    __device__ __forceinline__ float av(int j, int, const RowStats &) const { return avv[j]; }    // after put_av
    __device__ __forceinline__ float h(int j, int, const RowStats &, const HeadGrad &) const { return hv[j]; }
    __device__ __forceinline__ void put_e(int j, float e, float a) { qv[j] = e, avv[j] = a; }
    __device__ __forceinline__ void put_q(int j, float v) { qv[j] = v; }
    __device__ __forceinline__ void put_av(int j, float v) { avv[j] = v; }
    __device__ __forceinline__ void put_h(int j, float v) { hv[j] = v; }
};

// One wave, one row, in two steps.  A lane adds its entries in ascending k; row sums and maxima go through wave_sum / wave_max.
// row_stats: the row statistics, in every lane.
template <typename Row>
__device__ __forceinline__ RowStats row_stats(Row &row) {
    RowStats r;
    float mq = -INFINITY, ma = -INFINITY;
    row.each([&](int j, int k) {
        mq = fmaxf(mq, masked_logit(row.x(j, k), row.m(j, k)));
        ma = fmaxf(ma, row.x(j, k));
    });
    r.mq = wave_max(mq);
    r.ma = wave_max(ma);
    float sq = 0.0f, sa = 0.0f;
    row.each([&](int j, int k) {
        const float e = r.eq(row.x(j, k), row.m(j, k)), a = r.ea(row.x(j, k));
        row.put_e(j, e, a);
        sq += e;
        sa += a;
    });
    r.sq = wave_sum(sq);
    r.sa = wave_sum(sa);
    float tot = 0.0f;
    row.each([&](int j, int k) {
        const float q = row.eq(j, k, r) / r.sq;
        row.put_q(j, q);
        tot += q + kProbFloor;
    });
    r.tot = wave_sum(tot);
    return r;
}
// row_terms: ent (with ENT) and bad in every lane, and with GRAD the gradient into g[0 .. M).
template <bool ENT, bool GRAD, typename Row>
__device__ __forceinline__ void row_terms(Row &row, const RowStats &r, const HeadGrad &w, float *g, float &ent, float &bad) {
    float h = 0.0f, b = 0.0f, c = 0.0f;   // entropy, bad mass, sum_j p_j h_j
    row.each([&](int j, int k) {
        const float p = r.p(row.q(j, k, r));
        const float lg = clamp_log(p);
        if constexpr (ENT) h -= p * lg;
        const float av = row.ea(j, k, r) / r.sa;
        row.put_av(j, av);
        b += av * (1.0f - row.m(j, k));
        if constexpr (GRAD) {
            const float hk = head_hk(k == w.act, p, lg, w.gl, w.ge);
            row.put_h(j, hk);
            c += p * hk;
        }
    });
    if constexpr (ENT) h = wave_sum(h);
    b = wave_sum(b);
    if constexpr (GRAD) {
        c = wave_sum(c);
        float v = 0.0f;   // sum_j q_j u_j,  u_j = (h_j - c) / tot
        row.each([&](int j, int k) { v += row.q(j, k, r) * (row.h(j, k, r, w) - c) / r.tot; });
        v = wave_sum(v);
        row.each([&](int j, int k) {
            const float u = (row.h(j, k, r, w) - c) / r.tot;
            g[k] = row.q(j, k, r) * (u - v) + w.gb * row.av(j, k, r) * ((1.0f - row.m(j, k)) - b);
        });
    }
    ent = h;
    bad = b;
}

__global__ __launch_bounds__(256) void masked_eval_fwd_kernel(const float *logits, const float *mask, const int64_t *action,
                                                              float *logp, float *entropy, float *bad, int E, int M) {
    const int lane = threadIdx.x & (kWave - 1);
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const float *x = logits + (size_t)e * M, *m = mask + (size_t)e * M;
    MemRow row(x, m, M, lane);
    float h, b;
    const RowStats r = row_stats(row);
    row_terms<true, false>(row, r, HeadGrad{}, nullptr, h, b);
    if (lane == 0) {
        logp[e] = action_logp(x, m, M, action[e], r);
        entropy[e] = h;
        bad[e] = b;
    }
}

__global__ __launch_bounds__(256) void masked_eval_bwd_kernel(const float *logits, const float *mask, const int64_t *action,
                                                              const float *g_logp, const float *g_ent, const float *g_bad,
                                                              float *grad, int E, int M) {
    const int lane = threadIdx.x & (kWave - 1);
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    MemRow row(logits + (size_t)e * M, mask + (size_t)e * M, M, lane);
    const RowStats r = row_stats(row);
    const HeadGrad w{action[e], g_logp[e], g_ent[e], g_bad[e]};   // per-row weights
    float h, b;
    row_terms<false, true>(row, r, w, grad + (size_t)e * M, h, b);
}

// One wave draws a uniform-feasible entry of mask row r, that of the bin with global id env_id_base + bin, into actions[r] (0
// when nothing is feasible).
template <typename Bin>
__device__ __forceinline__ void sample_row_wave(const float *mask, int64_t *actions, int r, int M, int64_t env_id_base, Bin bin,
                                                uint64_t seed, uint64_t step, int lane) {
    const float *m = mask + (size_t)r * M;
    const int per = (M + kWave - 1) / kWave;
    const int b = min(lane * per, M), en = min(b + per, M);
    int cnt = 0;
    for (int k = b; k < en; ++k) cnt += (m[k] != 0.0f);
    const int incl = wave_scan_incl(cnt, lane);
    const int total = __shfl(incl, kWave - 1, kWave);
    if (total == 0) {
        if (lane == 0) actions[r] = 0;
        return;
    }
    int pick = (int)__umulhi(mix32(mix32_base(seed, step), (uint32_t)(env_id_base + bin)), (uint32_t)total);
    const int excl = incl - cnt;
    if (pick >= excl && pick < incl) {
        pick -= excl;
        for (int k = b; k < en; ++k)
            if (m[k] != 0.0f) {
                if (pick == 0) {
                    actions[r] = k;
                    break;
                }
                --pick;
            }
    }
}

// Fallback for rows that are not a multiple of 4 floats or longer than 16 * 8 quads: one wave per bin.
__global__ __launch_bounds__(256) void sample_kernel_generic(const float *mask, int64_t *actions, int E, int M,
                                                             int64_t env_id_base, uint64_t seed, uint64_t step) {
    const int lane = threadIdx.x & (kWave - 1);
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    sample_row_wave(mask, actions, e, M, env_id_base, e, seed, step, lane);
}

// The draw of a cell-scan subset step (bpp_step_subset with next_action): row i of the compact mask belongs to bin ids[i].
__global__ __launch_bounds__(256) void sample_ids_kernel(const float *mask, int64_t *actions, const int64_t *ids, int n, int M,
                                                         int64_t env_id_base, uint64_t seed, uint64_t step) {
    const int lane = threadIdx.x & (kWave - 1);
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    sample_row_wave(mask, actions, i, M, env_id_base, ids[i], seed, step, lane);
}

