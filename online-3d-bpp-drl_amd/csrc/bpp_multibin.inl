// bpp_multibin.inl -- the multi-bin packing of include/bpp_multibin.h (multi_bin/multi_bin.py), included at the end of
// bpp_kernels.hip so that the library stays one translation unit (and under its `fp contract(off)`).
//
// emit and choose give every slot one wave.  emit stages the pallet's heightmap in LDS once; lane j then owns cell quads
// j, j + 64, ... of the slot's K windows (flattened), writes the four planes of those cells with dwordx4 stores and the
// window mask bytes with one dword store per quad, the mask from the env's own "utils" rule (scan_window + feasible).
// choose walks the K windows in order: per window a softmax max / sum, the feasible count and the first masked argmax,
// reduced with shuffles, then lane 0 adds the window to the float64 advantage scan.  commit and clear are per slot.
namespace {

constexpr int kMBMaxK = BPP_MULTIBIN_MAX_K;

// A pallet's record of one window (multi_bin.py's past_rewards[label][-1], evaluations[label][-1]).
struct MBWin {
    double reward;     // last reward, valid when has
    double value;      // last value
    int64_t has;       // past_rewards[label] is not empty
};
static_assert(sizeof(MBWin) == 24, "MBWin layout");

// A slot's pending decision (16 bytes).
struct MBSlot {
    int32_t ok;        // ids[i] lies in [0, E)
    int32_t bin;
    uint32_t item;     // the item the rows were emitted for: x | y << 8 | z << 16
    int32_t window;    // chosen window, -1: none, -2: nothing to commit
};
static_assert(sizeof(MBSlot) == 16, "MBSlot layout");

struct MBArgs {
    int32_t n, K, Ky, w, w2, s, mstride, W, L, H, A, E;
    double bin_num, binvol;
    const int64_t *ids;
    MBWin *state;
    MBSlot *slots;
    uint8_t *masks;       // [n][K][mstride]
    const uint8_t *hmap;
    const bpp_env_state *bins;
};

__global__ __launch_bounds__(kWave * kSearchWaves) void multibin_emit_kernel(const MBArgs a, float *obs) {
    static __shared__ __attribute__((aligned(16))) uint8_t hs[kSearchWaves][kMaxArea];
    SEARCH_SLOT_PROLOGUE(a)
    const int64_t id = a.ids[i];
    MBSlot *sl = a.slots + i;
    if (!bin_in_range(id, a.E)) {
        if (lane == 0) *sl = MBSlot{0, 0, 0u, -2};
        return;
    }
    const int e = (int)id;
    uint8_t *h = hs[wv];
    const uint8_t *hm = a.hmap + (size_t)e * a.A;
    if ((a.A & 3) == 0)
        for (int c = lane * 4; c < a.A; c += 4 * kWave) *(uint32_t *)(h + c) = *(const uint32_t *)(hm + c);
    else
        for (int c = lane; c < a.A; c += kWave) h[c] = hm[c];
    const uint32_t it = a.bins[e].item_cur;
    wave_sync();
    const int x = it & 255u, y = (it >> 8) & 255u, z = (it >> 16) & 255u;
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    const int w = a.w, w2 = a.w2, Q = (w2 + 3) >> 2;
    const bool vec = (w2 & 3) == 0;
    for (int q = lane; q < a.K * Q; q += kWave) {
        const int k = q / Q, c0 = (q - k * Q) * 4;
        const int kx = k / a.Ky;
        const int dx = kx * a.s, dy = (k - kx * a.Ky) * a.s;
        float hv[4];
        uint32_t mbits = 0u;
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            hv[j] = 0.0f;
            if (c >= w2) continue;
            const int px = c / w, py = c - px * w;
            const int gx = dx + px, gy = dy + py;
            hv[j] = (float)h[gx * a.L + gy];
            // check_box in the w x w x H window (acktr/utils.py:8-35): the footprint stays inside the window
            if (px + x <= w && py + y <= w && feasible(scan_window(h, a.L, gx, gy, x, y), x * y, z, a.H, BPP_RULE_UTILS))
                mbits |= 1u << (8 * j);
        }
        float *row = obs + ((size_t)i * a.K + k) * 4 * w2;
        // store_obs_quad's stores, written out: through the shared function this kernel's code came out 17 instructions longer
        // and a decision of 65 536 pallets 1.7 % slower (profiles/search_common_ab.json)
        if (vec) {
            *(float4 *)(row + c0) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            *(float4 *)(row + w2 + c0) = make_float4(fx, fx, fx, fx);
            *(float4 *)(row + 2 * w2 + c0) = make_float4(fy, fy, fy, fy);
            *(float4 *)(row + 3 * w2 + c0) = make_float4(fz, fz, fz, fz);
        } else {
            for (int j = 0; j < 4 && c0 + j < w2; ++j) {
                row[c0 + j] = hv[j];
                row[w2 + c0 + j] = fx;
                row[2 * w2 + c0 + j] = fy;
                row[3 * w2 + c0 + j] = fz;
            }
        }
        *(uint32_t *)(a.masks + ((size_t)i * a.K + k) * a.mstride + c0) = mbits;
    }
    if (lane == 0) *sl = MBSlot{1, e, it, -2};
}

__global__ __launch_bounds__(kWave * kSearchWaves) void multibin_choose_kernel(const MBArgs a, const float *value, const float *logits,
                                                                            int64_t *action, double *adv, int32_t *window) {
    SEARCH_SLOT_PROLOGUE(a)
    MBSlot *sl = a.slots + i;
    const MBSlot s = *sl;
    if (!s.ok) {
        if (lane == 0) action[i] = BPP_ACTION_NOOP, adv[i] = 0.0, window[i] = -1;
        return;
    }
    const int w2 = a.w2;
    MBWin *rec = a.state + (size_t)s.bin * a.K;
    double max_adv = -1e8;
    int best_k = -1, best_c = 0;
    for (int k = 0; k < a.K; ++k) {
        const float *lg = logits + ((size_t)i * a.K + k) * w2;
        const uint8_t *mk = a.masks + ((size_t)i * a.K + k) * a.mstride;
        float mx, sum;
        int cnt = 0;
        row_softmax_stats(lg, w2, lane, mx, sum, [&](int c, float) { cnt += mk[c]; });
        cnt = wave_sum(cnt);
        if (cnt == 0 || cnt == w2) continue;                    // the mask (with its fallback) sums to w^2: skipped
        float best = -1.0f;
        int bi = 0;
        for (int c = lane; c < w2; c += kWave) {
            const float p = mk[c] ? expf(lg[c] - mx) / sum : 0.0f;     // poss * mask
            if (p > best) best = p, bi = c;
        }
        wave_argmax(best, bi, false);                            // np.argmax: the first maximum
        if (lane == 0) {
            const MBWin r = rec[k];
            const double v = (double)value[(size_t)i * a.K + k];
            const double cur = r.has ? a.bin_num * r.reward + (v - r.value) : -0.2;
            if (cur > max_adv) max_adv = cur, best_k = k, best_c = bi;
        }
    }
    if (lane != 0) return;
    if (best_k < 0) {                                            // no window: action 0, label (0, 0)
        action[i] = 0;
        adv[i] = max_adv;
        window[i] = -1;
        sl->window = -1;
        return;
    }
    const int kx = best_k / a.Ky;
    const int lx = kx * a.s + best_c / a.w, ly = (best_k - kx * a.Ky) * a.s + best_c % a.w;
    rec[best_k].value = (double)value[(size_t)i * a.K + best_k];  // evaluations[max_label].append(new_value)
    action[i] = (int64_t)lx * a.L + ly;
    adv[i] = max_adv;
    window[i] = best_k;
    sl->window = best_k;
}

__global__ void multibin_commit_kernel(const MBArgs a, const uint8_t *step_done) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n) return;
    MBSlot *sl = a.slots + i;
    const MBSlot s = *sl;
    if (!s.ok || s.window == -2) return;
    MBWin *rec = a.state + (size_t)s.bin * a.K;
    if (step_done[i]) {                                          // the episode ended: test() starts new dicts
        for (int k = 0; k < a.K; ++k) rec[k] = MBWin{0.0, 0.0, 0};
    } else {
        const double r = volume_reward(item_volume(s.item), a.binvol);
        if (s.window >= 0) {
            rec[s.window].reward = r;
            rec[s.window].has = 1;
        } else if (rec[0].has) {                                 // past_rewards[(0, 0)].append (KeyError without history)
            rec[0].reward = r;
        }
    }
    sl->window = -2;
}

__global__ void multibin_clear_kernel(const MBArgs a, const int64_t *ids, int n) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n * a.K) return;
    const int j = t / a.K, k = t - j * a.K;
    const int64_t id = ids ? ids[j] : (int64_t)j;
    if (!bin_in_range(id, a.E)) return;
    a.state[(size_t)id * a.K + k] = MBWin{0.0, 0.0, 0};
}

struct MBLayout {
    int64_t K, state, masks, total;
    int32_t Ky, mstride;
};

// Geometry of the windows and the buffers; 0 or an error (messages name `who`).
int multibin_layout(int W, int L, int w, int s, int64_t n, int64_t E, const ArgCheck &ck, MBLayout &l) {
    if (W <= 0 || L <= 0 || W * L > kMaxArea) return ck.bad("pallet W * L must be in 1 .. 1024");
    if (w < 1 || w > W || w > L) return ck.bad("window side w must be in 1 .. min(W, L)");
    if (w * w > kMaxArea) return ck.bad("window area w * w must be at most 1024");
    if (s < 1) return ck.bad("stride s must be at least 1");
    if (n < 0 || E < 0) return ck.bad("negative n or E");
    const int Kx = (W - w) / s + 1, Ky = (L - w) / s + 1;
    l.K = (int64_t)Kx * Ky;
    if (l.K > kMBMaxK) return ck.bad("more windows than BPP_MULTIBIN_MAX_K (256)");
    l.Ky = Ky;
    l.mstride = (w * w + 15) / 16 * 16;
    l.state = E * l.K * (int64_t)sizeof(MBWin);
    l.masks = (n * (int64_t)sizeof(MBSlot) + 255) / 256 * 256;
    l.total = l.masks + n * l.K * l.mstride;
    return 0;
}

// Everything a multi-bin call checks before device work; fills the kernel arguments.
int multibin_args(const bpp_batch *b, const bpp_multibin *m, const ArgCheck &ck, MBArgs &a) {
    int rc = check_search_batch(b, m, ck, "multi-bin packing supports pallets without rotation only", false);
    if (rc) return rc;
    MBLayout l;
    rc = multibin_layout(b->W, b->L, m->w, m->s, m->n, b->num_envs, ck, l);
    if (rc) return rc;
    if (m->K != l.K) return ck.bad("K does not match the geometry (use bpp_multibin_sizes)");
    if (m->n > 0 && (!m->ids || !m->work)) return ck.bad("NULL pointer");
    if (!m->state) return ck.bad("NULL state");
    if (((uintptr_t)m->ids & 7u) || ((uintptr_t)m->state & 7u) || ((uintptr_t)m->work & 15u))
        return ck.bad("ids / state must be 8-byte aligned, work 16-byte aligned");
    a.n = m->n, a.K = (int32_t)l.K, a.Ky = l.Ky, a.w = m->w, a.w2 = m->w * m->w, a.s = m->s, a.mstride = l.mstride;
    a.W = b->W, a.L = b->L, a.H = b->H, a.A = b->W * b->L, a.E = b->num_envs;
    a.bin_num = (double)(b->W * b->L) / (double)(m->w * m->w);   // (plain.shape[0] * plain.shape[1]) / (w * w)
    a.binvol = (double)b->W * b->L * b->H;
    a.ids = m->ids;
    a.state = (MBWin *)m->state;
    a.slots = (MBSlot *)m->work;
    a.masks = (uint8_t *)m->work + l.masks;
    a.hmap = b->hmap;
    a.bins = b->state;
    return 0;
}

}  // namespace

extern "C" {

int bpp_multibin_sizes(int32_t W, int32_t L, int32_t w, int32_t s, int32_t n, int32_t E, int64_t out[3]) {
    const ArgCheck ck{"bpp_multibin_sizes"};
    if (!out) return ck.bad("NULL pointer");
    MBLayout l;
    const int rc = multibin_layout(W, L, w, s, n, E, ck, l);
    if (rc) return rc;
    out[0] = l.K;
    out[1] = l.state;
    out[2] = l.total;
    return 0;
}

int bpp_multibin_emit(const bpp_batch *b, const bpp_multibin *m, float *obs, void *stream) {
    MBArgs a;
    const ArgCheck ck{"bpp_multibin_emit"};
    if (const int rc = multibin_args(b, m, ck, a)) return rc;
    if (a.n > 0 && !obs) return ck.bad("NULL obs");
    if ((uintptr_t)obs & 15u) return ck.bad("obs must be 16-byte aligned");
    return launch_slots(multibin_emit_kernel, a.n, stream, a, obs);
}

int bpp_multibin_choose(const bpp_batch *b, const bpp_multibin *m, const float *value, const float *logits, int64_t *action,
                        double *adv, int32_t *window, void *stream) {
    MBArgs a;
    const ArgCheck ck{"bpp_multibin_choose"};
    if (const int rc = multibin_args(b, m, ck, a)) return rc;
    if (a.n > 0 && (!value || !logits || !action || !adv || !window)) return ck.bad("NULL pointer");
    if (((uintptr_t)value & 3u) || ((uintptr_t)logits & 3u) || ((uintptr_t)action & 7u) || ((uintptr_t)adv & 7u) ||
        ((uintptr_t)window & 3u))
        return ck.bad("misaligned buffer");
    return launch_slots(multibin_choose_kernel, a.n, stream, a, value, logits, action, adv, window);
}

int bpp_multibin_commit(const bpp_batch *b, const bpp_multibin *m, const uint8_t *step_done, void *stream) {
    MBArgs a;
    const ArgCheck ck{"bpp_multibin_commit"};
    if (const int rc = multibin_args(b, m, ck, a)) return rc;
    if (a.n > 0 && !step_done) return ck.bad("NULL step_done");
    return launch_items(multibin_commit_kernel, a.n, stream, a, step_done);
}

int bpp_multibin_clear(const bpp_batch *b, const bpp_multibin *m, const int64_t *ids, int32_t n, void *stream) {
    MBArgs a;
    const ArgCheck ck{"bpp_multibin_clear"};
    if (const int rc = multibin_args(b, m, ck, a)) return rc;
    if (!ids) n = a.E;
    if (n < 0) return ck.bad("negative n");
    if ((uintptr_t)ids & 7u) return ck.bad("ids must be 8-byte aligned");
    return launch_items(multibin_clear_kernel, (int64_t)n * a.K, stream, a, ids, n);
}

}  // extern "C"
