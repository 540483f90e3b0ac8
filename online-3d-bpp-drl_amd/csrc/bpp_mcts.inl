// bpp_mcts.inl -- the batched MCTS of include/bpp_mcts.h (MCTS/monteCarlo.py, MCTS/node.py, driven as mcts_test.py:14-65),
// included at the end of bpp_kernels.hip so that the library stays one translation unit.
//
// One wave per search slot.  The tree walk is wave-uniform work done by lane 0 on the bin's node pool in global memory,
// in float64 without FMA contraction; the lanes do the A-cell and per-child work: the observation row, the feasibility
// mask and the child records of an expansion, the softmax, choose_best's values (into LDS, for lane 0's order-dependent
// scan) and the pool compaction.  Every draw of the bin's numpy-legacy MT19937 stream is made by the whole wave (the
// twist is wave-wide, in place in global memory), so the stream position stays wave-uniform.
//
// State layout (bpp_mcts_sizes): MBin [E] (192 bytes), then MT words [E][kMtStride], then MRec pools [E][2][cap].
namespace {

constexpr int kMctsMaxK = BPP_MCTS_MAX_K;
constexpr int kMtStride = 640;      // 624 words, padded to a multiple of 64 bytes

// A pool record: a child (node.py Node), or the header of a block of children (w: the node value, n: the child count).
struct MRec {
    double w;          // Node.w
    double p;          // Node.p
    int32_t n;         // Node.n
    int32_t block;     // the node's children: index of their header record in the same pool half, -1: not expanded
    uint16_t action;
    uint8_t term;      // Node.terminated
    uint8_t pad;
    uint32_t vol;      // x*y*z of the item the step into this node placed; 0: no reward (not stepped yet, or failed)
};
static_assert(sizeof(MRec) == 32, "MRec layout");

enum { kIdle = 0, kDescend = 1, kExpand = 2, kRollout = 3, kBackup = 4 };

struct MScal {
    int32_t tree;      // the bin has a root (record 0 of pool half `half`)
    int32_t half;
    int32_t nrec;      // records in use in that half
    int32_t mtpos;     // position in the MT19937 state (624: twist before the next draw)
    int32_t mode;      // this simulation: kIdle .. kBackup
    int32_t depth;     // depth of the current node (path[depth])
    int32_t stepped;   // the last bpp_step_subset stepped the scratch bin with our action: its commit is pending
    uint32_t item;     // the item that step placed
    int32_t rb, ri;    // rollout: box_num, index of the pending step
    int32_t pick;      // finish: the record of the chosen child (-1: none)
    int32_t ovf;       // the pool half ran out during this decision
    double value;      // leaf value (kBackup) / last evaluate's value (kRollout)
    int32_t row;       // the last emit wrote this slot's row
    int32_t leaf;      // the leaf was expanded in this simulation (its node value is set at the backup)
};
static_assert(sizeof(MScal) == 64, "MScal layout");

struct MBin {
    MScal s;
    int32_t path[kMctsMaxK];     // records from the root (path[0] = 0) to the current node
    uint32_t rvol[kMctsMaxK];    // the rollout's reward stack, as item volumes
};
static_assert(sizeof(MBin) == 192, "MBin layout");

struct MctsArgs {
    int32_t n, k, S, max_depth, rollout, cap, A, W, L, H, E;
    double credit, zeta, binvol;
    const int64_t *ids, *scratch;
    MBin *bins;
    uint32_t *mt;
    MRec *pool;
    int32_t *overflow;
    const uint8_t *hmap;
    bpp_env_state *state;
};

__device__ __forceinline__ MRec *mcts_half(const MctsArgs &a, int e, int half) { return a.pool + ((size_t)e * 2 + half) * a.cap; }

__device__ __forceinline__ void mcts_sync() { twist_sync<true>(); }

// ---- numpy's legacy RandomState on the bin's MT19937 (include/bpp_gen.inl: bpp_npmt_*), wave-wide ----------------------
// (The same rounds as stream_wave_twist's, bpp_stream_gen.inl.  They are not shared: built from one function, the stream
// kernels' instructions came out in another order, profiles/search_common_resource_usage.txt.)
__device__ __forceinline__ void mt_twist_wave(uint32_t *mt, int lane) {
    mcts_sync();
    for (int k0 = 0; k0 < 624; k0 += kWave) {     // in place, 64 words at a time: mt[k + 1] is still old, mt[k - 227] new
        const int k = k0 + lane;
        uint32_t x = 0, y = 0, z = 0;
        if (k < 624) {
            x = mt[k];
            y = mt[k + 1 < 624 ? k + 1 : 0];
            z = mt[k + 397 < 624 ? k + 397 : k - 227];
        }
        mcts_sync();
        if (k < 624) {
            const uint32_t v = (x & 0x80000000u) | (y & 0x7fffffffu);
            mt[k] = z ^ (v >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
        }
        mcts_sync();
    }
}

// Every lane of the wave calls these with the same pos.
__device__ __forceinline__ uint32_t mt_draw(uint32_t *mt, int &pos, int lane) {
    if (pos >= 624) {
        mt_twist_wave(mt, lane);
        pos = 0;
    }
    const uint32_t y = mt[pos];
    ++pos;
    return mt_temper(y);
}
// np.random.randint(0, n): no draw for n == 1, else masked rejection on 32-bit words
__device__ __forceinline__ uint32_t mt_below(uint32_t *mt, int &pos, int lane, uint32_t n) {
    const uint32_t rng = n - 1u;
    if (rng == 0u) return 0u;
    uint32_t mask = rng;
    mask |= mask >> 1, mask |= mask >> 2, mask |= mask >> 4, mask |= mask >> 8, mask |= mask >> 16;
    uint32_t v;
    do v = mt_draw(mt, pos, lane) & mask;
    while (v > rng);
    return v;
}
// np.random.random_sample()
__device__ __forceinline__ double mt_double(uint32_t *mt, int &pos, int lane) {
    const uint32_t x = mt_draw(mt, pos, lane) >> 5;
    const uint32_t y = mt_draw(mt, pos, lane) >> 6;
    return ((double)x * 67108864.0 + (double)y) / 9007199254740992.0;
}

// math.isclose(a, b, rel_tol=1e-5) (CPython's formula)
__device__ __forceinline__ bool py_isclose(double a, double b) {
    if (a == b) return true;
    if (isinf(a) || isinf(b)) return false;
    const double d = fabs(b - a);
    return d <= fabs(1e-5 * b) || d <= fabs(1e-5 * a);
}

// Lane 0: np.random.choice(len(p), p=p) with the uniform u already drawn: cdf = cumsum(float64(p)) sequentially,
// cdf /= cdf[-1], searchsorted(cdf, u, 'right').
template <typename T>
__device__ __forceinline__ int choice_scan(const T *p, int cnt, double u) {
    double tot = 0.0;
    for (int j = 0; j < cnt; ++j) tot += (double)p[j];
    double run = 0.0;
    for (int j = 0; j < cnt; ++j) {
        run += (double)p[j];
        if (run / tot > u) return j;
    }
    return cnt - 1;
}

// model_loader.evaluate(obs, False)'s pvec: exp(x - max) / sum in float32 (IEEE division), into LDS pv[0..A).
__device__ __forceinline__ void mcts_softmax(const MctsArgs &a, const float *lg, float *pv, int lane) {
    float mx, sum;
    row_softmax_stats(lg, a.A, lane, mx, sum, [&](int c, float v) { pv[c] = v; });
    for (int c = lane; c < a.A; c += kWave) pv[c] = pv[c] / sum;
    wave_sync();
}

// Lane 0: commit the step of the scratch bin that the previous launch chose (step_done[i]).
__device__ __forceinline__ void mcts_commit(const MctsArgs &a, MScal &s, MBin *bp, MRec *P, bool done) {
    if (!s.stepped) return;
    s.stepped = 0;
    if (s.mode == kDescend) {                                    // monteCarlo.py:64-75
        MRec &c = P[bp->path[s.depth + 1]];
        c.vol = done ? 0u : item_volume(s.item);
        s.depth += 1;
        if (done) {
            if (!c.term) c.term = 1, c.p = 0.0;
            s.value = 0.0;
            s.mode = kBackup;
        }
    } else if (s.mode == kRollout) {                             // node.py:156-166
        if (done) {
            s.value = 0.0;
            s.mode = kBackup;
        } else if (s.ri + 1 < s.rb) {
            bp->rvol[s.ri] = item_volume(s.item);
            s.ri += 1;
        } else {
            s.mode = kBackup;                                    // the last step only decides `done`
        }
    }
}

// Lane 0: MCTree.select's tests at the current node (monteCarlo.py:42-60).  Returns 1 when choose_best is next.
__device__ __forceinline__ int mcts_classify(const MctsArgs &a, MScal &s, MBin *bp, MRec *P) {
    const MRec &nd = P[bp->path[s.depth]];
    if (nd.term) {
        s.value = 0.0;
        s.mode = kBackup;
        return 0;
    }
    if (nd.block < 0) {
        s.mode = kExpand;
        return 0;
    }
    if (s.depth == a.max_depth) {
        s.value = P[nd.block].w;
        s.mode = kBackup;
        return 0;
    }
    return 1;
}

__device__ __forceinline__ void mcts_start(const MctsArgs &a, MScal &s, MBin *bp) {
    s.mode = s.tree && !s.ovf ? kDescend : kIdle;
    s.depth = 0;
    s.stepped = 0;
    s.row = 0;
    s.leaf = 0;
    s.ri = 0;
    s.rb = 0;
    bp->path[0] = 0;
}

// Node.choose_best(c = 1) over the children of record `node`, the whole wave: the values lane-parallel into LDS, the
// order-dependent scan by lane 0, the tie break with the bin's stream.  Returns the chosen child's record.
__device__ __forceinline__ int mcts_choose(const MctsArgs &a, MRec *P, int node, uint32_t *mt, int &pos, int lane, double *vals,
                                          uint16_t *ties) {
    const MRec par = P[node];
    const int blk = par.block, cnt = P[blk].n;
    const double sq = sqrt((double)par.n);
    const double pq = par.n > 0 ? par.w / (double)par.n : 0.0;
    for (int j = lane; j < cnt; j += kWave) {
        const MRec c = P[blk + 1 + j];
        const double u = (c.p * sq) / (double)(c.n + 1);        // get_u_value
        vals[j] = c.n > 0 ? ((c.w / (double)c.n) - pq) + u : 0.0 + u;
    }
    wave_sync();
    int nt = 0;
    if (lane == 0) {
        double mx = -1000000007.0;                               // -INF of node.py
        for (int j = 0; j < cnt; ++j) {
            const double v = vals[j];
            if (py_isclose(v, mx)) {
                ties[nt++] = (uint16_t)j;
            } else if (v > mx) {
                mx = v;
                nt = 0;
                ties[nt++] = (uint16_t)j;
            }
        }
    }
    wave_sync();
    nt = __shfl(nt, 0, kWave);
    const int t = (int)mt_below(mt, pos, lane, (uint32_t)nt);
    const int pick = ties[t];
    wave_sync();
    return blk + 1 + pick;
}

// The observation row of scratch bin sid (cur_observation: heights, then the item's x, y, z planes).
__device__ __forceinline__ void mcts_row(const MctsArgs &a, int sid, int i, float *obs, int lane) {
    const uint32_t it = a.state[sid].item_cur;
    const float fx = (float)(it & 255u), fy = (float)((it >> 8) & 255u), fz = (float)((it >> 16) & 255u);
    const uint8_t *hm = a.hmap + (size_t)sid * a.A;
    float *row = obs + (size_t)i * 4 * a.A;
    for (int c0 = lane * 4; c0 < a.A; c0 += 4 * kWave) {
        float h[4];
        for (int q = 0; q < 4; ++q) h[q] = c0 + q < a.A ? (float)hm[c0 + q] : 0.0f;
        store_obs_quad(row, a.A, c0, h, fx, fy, fz);
    }
}

// bpp_mcts_begin: one thread per slot.
__global__ void mcts_begin_kernel(const MctsArgs a) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n) return;
    int e, sid;
    if (!slot_bins(a, i, e, sid)) return;
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    if (!s.tree) {                                               // MCTree.__init__: root = PutNode(None, 1.0)
        MRec r;
        r.w = 0.0, r.p = 1.0, r.n = 0, r.block = -1, r.action = 0, r.term = 0, r.pad = 0, r.vol = 0u;
        mcts_half(a, e, s.half)[0] = r;
        s.tree = 1;
        s.nrec = 1;
    }
    s.mode = kIdle, s.stepped = 0, s.row = 0, s.leaf = 0, s.ovf = 0, s.pick = -1;
    bp->s = s;
}

// bpp_mcts_select: level `level` of the descent.
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_select_kernel(const MctsArgs a, int level, const uint8_t *step_done,
                                                                          int64_t *actions) {
    static __shared__ double s_vals[kSearchWaves][kMaxArea];
    static __shared__ uint16_t s_ties[kSearchWaves][kMaxArea];
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    MRec *P = mcts_half(a, e, s.half);
    int go = 0;
    if (lane == 0) {
        if (level == 0) mcts_start(a, s, bp);
        else if (step_done) mcts_commit(a, s, bp, P, step_done[i] != 0);
        if (s.mode == kDescend) go = mcts_classify(a, s, bp, P);
    }
    go = __shfl(go, 0, kWave);
    int64_t act = BPP_ACTION_NOOP;
    if (go) {
        int pos = __shfl(s.mtpos, 0, kWave);
        const int node = __shfl(bp->path[__shfl(s.depth, 0, kWave)], 0, kWave);
        const int child = mcts_choose(a, P, node, a.mt + (size_t)e * kMtStride, pos, lane, s_vals[wv], s_ties[wv]);
        if (lane == 0) {
            s.mtpos = pos;
            bp->path[s.depth + 1] = child;
            s.item = a.state[sid].item_cur;
            s.stepped = 1;
            act = P[child].action;
        }
    }
    if (lane == 0) {
        actions[i] = act;
        bp->s = s;
    }
}

// bpp_mcts_emit: commit, then the row of every slot whose leaf is expanded (rlevel 0) or whose rollout goes on.
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_emit_kernel(const MctsArgs a, int rlevel, const uint8_t *step_done,
                                                                        float *obs) {
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) return;
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    MRec *P = mcts_half(a, e, s.half);
    int emit = 0;
    if (lane == 0) {
        if (rlevel == 0 && a.max_depth == 0) mcts_start(a, s, bp);
        else if (step_done) mcts_commit(a, s, bp, P, step_done[i] != 0);
        if (rlevel == 0 && s.mode == kDescend) mcts_classify(a, s, bp, P);
        emit = (rlevel == 0 && s.mode == kExpand) || (rlevel > 0 && s.mode == kRollout);
        s.row = emit;
        bp->s = s;
    }
    emit = __shfl(emit, 0, kWave);
    if (emit) mcts_row(a, sid, i, obs, lane);
}

// bpp_mcts_expand: PutNode.expand (node.py:92-137) of the slots whose row was emitted at rollout level 0.
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_expand_kernel(const MctsArgs a, const float *value, const float *logits,
                                                                          int64_t *actions) {
    static __shared__ float s_pv[kSearchWaves][kMaxArea];
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    if (!(s.row && s.mode == kExpand)) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    MRec *P = mcts_half(a, e, s.half);
    float *pv = s_pv[wv];
    mcts_softmax(a, logits + (size_t)i * a.A, pv, lane);
    // sim_env.get_possible_position() (bin3D.py:72-93): Space.check_box inside the bin, all ones when nothing fits
    const uint32_t it = a.state[sid].item_cur;
    const int x = it & 255u, y = (it >> 8) & 255u, z = (it >> 16) & 255u;
    const uint8_t *h = a.hmap + (size_t)sid * a.A;
    int valid = 0;
    for (int c0 = 0; c0 < a.A; c0 += kWave) {
        const int c = c0 + lane;
        bool f = false;
        if (c < a.A) {
            const int px = c / a.L, py = c - px * a.L;
            f = px + x <= a.W && py + y <= a.L && feasible(scan_window(h, a.L, px, py, x, y), x * y, z, a.H, BPP_RULE_SPACE);
        }
        valid += __popcll(__ballot(f));
    }
    const bool all = valid == 0;
    if (all) valid = a.A;
    const int need = 1 + valid;
    if (s.nrec + need > a.cap) {                                 // the pool half ran out: this slot's search stops
        if (lane == 0) {
            atomicAdd(a.overflow, 1);
            s.ovf = 1;
            s.mode = kIdle;
            s.row = 0;
            bp->s = s;
            actions[i] = BPP_ACTION_NOOP;
        }
        return;
    }
    const int blk = s.nrec;
    const double fill = (1.0 - a.credit) * (1.0 / (double)valid);
    const float cf = (float)a.credit;
    int base = 0;
    for (int c0 = 0; c0 < a.A; c0 += kWave) {
        const int c = c0 + lane;
        bool f = false;
        if (c < a.A) {
            const int px = c / a.L, py = c - px * a.L;
            f = all || (px + x <= a.W && py + y <= a.L && feasible(scan_window(h, a.L, px, py, x, y), x * y, z, a.H, BPP_RULE_SPACE));
        }
        const unsigned long long bits = __ballot(f);
        if (f) {
            MRec r;
            r.w = 0.0;
            r.p = (double)(cf * pv[c]) + fill;                   // credit * pvec[a] in float32 (NEP 50), then float64
            r.n = 0, r.block = -1, r.action = (uint16_t)c, r.term = 0, r.pad = 0, r.vol = 0u;
            P[blk + 1 + base + __popcll(bits & ((1ull << lane) - 1ull))] = r;
        }
        base += __popcll(bits);
    }
    int64_t act = BPP_ACTION_NOOP;
    if (lane == 0) {
        MRec hd;
        hd.w = (double)value[i], hd.p = 0.0, hd.n = valid, hd.block = -1, hd.action = 0, hd.term = 0, hd.pad = 0, hd.vol = 0u;
        P[blk] = hd;
        P[bp->path[s.depth]].block = blk;
        s.nrec += need;
        s.value = (double)value[i];
        s.leaf = 1;
        s.row = 0;
        const int blen = a.k - s.depth;                          // len(box_size_list)
        const int r = a.rollout < 0 ? blen - 1 : a.rollout;
        if (r >= 1 && blen >= r + 1) {
            s.rb = r + 1;
            s.ri = 0;
            s.mode = kRollout;
        } else {
            s.mode = kBackup;
        }
    }
    const int roll = __shfl(s.mode, 0, kWave) == kRollout;
    if (roll) {                                                  // roll_out's first action, on the expansion's evaluate
        int pos = __shfl(s.mtpos, 0, kWave);
        wave_sync();
        const double u = mt_double(a.mt + (size_t)e * kMtStride, pos, lane);
        if (lane == 0) {
            s.mtpos = pos;
            act = choice_scan(pv, a.A, u);
            s.item = it;
            s.stepped = 1;
        }
    }
    if (lane == 0) {
        actions[i] = act;
        bp->s = s;
    }
}

// bpp_mcts_rollout: one more evaluate and np.random.choice of roll_out (node.py:151-160).
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_rollout_kernel(const MctsArgs a, const float *value, const float *logits,
                                                                           int64_t *actions) {
    static __shared__ float s_pv[kSearchWaves][kMaxArea];
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    if (!(s.row && s.mode == kRollout)) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    float *pv = s_pv[wv];
    mcts_softmax(a, logits + (size_t)i * a.A, pv, lane);
    int pos = s.mtpos;
    const double u = mt_double(a.mt + (size_t)e * kMtStride, pos, lane);
    if (lane == 0) {
        s.mtpos = pos;
        s.value = (double)value[i];
        s.row = 0;
        s.item = a.state[sid].item_cur;
        s.stepped = 1;
        actions[i] = choice_scan(pv, a.A, u);
        bp->s = s;
    }
}

// bpp_mcts_backup: the last commit, the rollout's value, MCTree.backup (monteCarlo.py:82-90).  One thread per slot.
__global__ void mcts_backup_kernel(const MctsArgs a, const uint8_t *step_done) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n) return;
    int e, sid;
    if (!slot_bins(a, i, e, sid)) return;
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    MRec *P = mcts_half(a, e, s.half);
    if (step_done) mcts_commit(a, s, bp, P, step_done[i] != 0);
    if (s.mode == kBackup) {
        double v = s.value;
        if (s.rb > 0)                                            // node.py:168-170
            for (int j = s.ri - 1; j >= 0; --j) v = volume_reward(bp->rvol[j], a.binvol) + v;
        if (s.leaf) P[P[bp->path[s.depth]].block].w = v;         // self.value = value
        for (int d = s.depth; d >= 0; --d) {
            MRec &r = P[bp->path[d]];
            v = volume_reward(r.vol, a.binvol) + v;
            r.n += 1;
            r.w += v;
        }
    }
    s.mode = kIdle;
    s.stepped = 0;
    s.row = 0;
    bp->s = s;
}

// bpp_mcts_finish: MCTree.play(zeta) and sample_action (monteCarlo.py:92-125).
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_finish_kernel(const MctsArgs a, int64_t *action, int32_t *visits) {
    static __shared__ double s_p[kSearchWaves][kMaxArea];
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) {
        if (lane == 0) action[i] = BPP_ACTION_NOOP, visits[i] = 0;
        return;
    }
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    MRec *P = mcts_half(a, e, s.half);
    const MRec root = P[0];
    if (!s.tree || root.block < 0) {                             // nothing was expanded (a pool that ran out at once)
        if (lane == 0) {
            action[i] = 0, visits[i] = root.n;
            s.pick = -1;
            bp->s = s;
        }
        return;
    }
    const int blk = root.block, cnt = P[blk].n;
    double *p = s_p[wv];
    int pick = 0;
    if (a.max_depth == 0) {                                      // max(next_nodes, key=p): the first maximum, no draw
        if (lane == 0) {
            double best = P[blk + 1].p;
            for (int j = 1; j < cnt; ++j)
                if (P[blk + 1 + j].p > best) best = P[blk + 1 + j].p, pick = j;
        }
    } else {
        // softmax(1 / zeta * log(visits + 1e-10)) in float64, then np.random.choice(actions, p=...)
        const double inv = 1.0 / a.zeta;
        double mx = -INFINITY;
        for (int j = lane; j < cnt; j += kWave) {
            const double x = inv * log((double)P[blk + 1 + j].n + 1e-10);
            p[j] = x;
            mx = fmax(mx, x);
        }
        mx = wave_max(mx);
        for (int j = lane; j < cnt; j += kWave) p[j] = exp(p[j] - mx);
        wave_sync();
        int pos = s.mtpos;
        const double u = mt_double(a.mt + (size_t)e * kMtStride, pos, lane);
        if (lane == 0) {
            double sum = 0.0;
            for (int j = 0; j < cnt; ++j) sum += p[j];
            for (int j = 0; j < cnt; ++j) p[j] = p[j] / sum;
            pick = choice_scan(p, cnt, u);
            s.mtpos = pos;
        }
    }
    if (lane == 0) {
        action[i] = P[blk + 1 + pick].action;
        visits[i] = root.n;
        s.pick = blk + 1 + pick;
        bp->s = s;
    }
}

// bpp_mcts_advance: MCTree.succeed (monteCarlo.py:127-139) -- the chosen child's subtree is copied, breadth first, into the
// other pool half, the child at record 0 with p = 1 -- or a dropped tree where the episode ended.
__global__ __launch_bounds__(kWave * kSearchWaves) void mcts_advance_kernel(const MctsArgs a, const uint8_t *done) {
    SEARCH_SLOT_BINS_PROLOGUE(a)
    if (!ok) return;
    MBin *bp = a.bins + e;
    MScal s = bp->s;
    wave_sync();
    if (done[i] || !s.tree || s.pick < 0) {
        if (lane == 0) {
            s.tree = 0;
            bp->s = s;
        }
        return;
    }
    const MRec *src = mcts_half(a, e, s.half);
    MRec *dst = mcts_half(a, e, s.half ^ 1);
    MRec r = src[s.pick];
    int next = 1;
    if (r.block >= 0) {
        const int len = 1 + src[r.block].n;
        for (int q = lane; q < len; q += kWave) dst[1 + q] = src[r.block + q];
        r.block = 1;
        next = 1 + len;
    }
    r.p = 1.0;
    if (lane == 0) dst[0] = r;
    mcts_sync();
    for (int bq = 1; bq < next;) {                               // the header of a copied block: relocate its children's blocks
        const int cnt = dst[bq].n;
        for (int j0 = 0; j0 < cnt; j0 += kWave) {
            const int j = j0 + lane;
            int sb = -1, sz = 0;
            if (j < cnt) {
                sb = dst[bq + 1 + j].block;
                if (sb >= 0) sz = 1 + src[sb].n;
            }
            int off = wave_scan_incl(sz, lane);                  // inclusive prefix of the block sizes over the lanes
            const int total = __shfl(off, kWave - 1, kWave);
            off -= sz;
            if (sb >= 0) dst[bq + 1 + j].block = next + off;
            unsigned long long has = __ballot(sb >= 0);
            while (has) {
                const int l = __ffsll(has) - 1;
                has &= has - 1ull;
                const int from = __shfl(sb, l, kWave), to = next + __shfl(off, l, kWave), len = __shfl(sz, l, kWave);
                for (int q = lane; q < len; q += kWave) dst[to + q] = src[from + q];
            }
            next += total;
            mcts_sync();
        }
        bq += 1 + cnt;
    }
    if (lane == 0) {
        s.half ^= 1;
        s.nrec = next;
        s.pick = -1;
        bp->s = s;
    }
}

// bpp_mcts_seed: np.random.seed(s) -- init_genrand -- for listed bins.  One thread per bin.
__global__ void mcts_seed_kernel(const MctsArgs a, const int64_t *ids, const uint32_t *seeds, int count) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= count) return;
    const int64_t id = ids[j];
    if (!bin_in_range(id, a.E)) return;
    uint32_t *mt = a.mt + (size_t)id * kMtStride;
    uint32_t v = seeds[j];
    mt[0] = v;
    for (int k = 1; k < 624; ++k) {
        v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)k;
        mt[k] = v;
    }
    a.bins[id].s.mtpos = 624;
}

// bpp_mcts_clear: drop the trees of listed bins (ids NULL: of every bin).  One thread per bin.
__global__ void mcts_clear_kernel(const MctsArgs a, const int64_t *ids, int count) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= count) return;
    const int64_t id = ids ? ids[j] : (int64_t)j;
    if (!bin_in_range(id, a.E)) return;
    a.bins[id].s.tree = 0;
}

int64_t mcts_cap(int k, int S, int max_depth, int A) { return 1 + (int64_t)(max_depth + 1) * S * (A + 1); }

int mcts_rollout_levels(int k, int max_depth, int rollout) {
    if (rollout == 0) return 0;
    if (rollout < 0) return k >= 2 ? k : 0;                      // depth 0: box_num = k, r = k - 1 >= 1
    return k >= rollout + 1 ? rollout + 1 : 0;
}

struct MctsLayout {
    int64_t bins, mt, pool, total, per_bin;
};

MctsLayout mcts_layout(int64_t E, int64_t cap) {
    MctsLayout l;
    l.bins = 0;
    l.mt = E * (int64_t)sizeof(MBin);
    l.pool = l.mt + E * kMtStride * 4;
    l.total = l.pool + E * 2 * cap * (int64_t)sizeof(MRec);
    l.per_bin = (int64_t)sizeof(MBin) + kMtStride * 4 + 2 * cap * (int64_t)sizeof(MRec);
    return l;
}

// Everything an MCTS call checks before device work; fills the kernel arguments.
int mcts_args(const bpp_batch *b, const bpp_mcts *m, const ArgCheck &ck, MctsArgs &a) {
    const int rc = check_search_batch(b, m, ck, "MCTS supports bins without rotation only", false);
    if (rc) return rc;
    if (m->k < 2 || m->k > kMctsMaxK) return ck.bad("k must be in 2 .. 16");
    if (m->n < 0) return ck.bad("negative n");
    if (m->sim_times < 1) return ck.bad("sim_times must be positive");
    if (m->max_depth < 0 || m->max_depth > m->k - 1) return ck.bad("max_depth must be in 0 .. k - 1");
    if (m->rollout_length < -1) return ck.bad("rollout_length must be -1, 0 or positive");
    if (!(m->credit >= 0.0 && m->credit <= 1.0)) return ck.bad("credit must be in [0, 1]");
    if (!(m->zeta > 0.0)) return ck.bad("zeta must be positive");
    const int A = b->W * b->L;
    if (m->cap != mcts_cap(m->k, m->sim_times, m->max_depth, A)) return ck.bad("cap must be the one bpp_mcts_sizes gives");
    if (!m->state || !m->overflow) return ck.bad("NULL state / overflow");
    if (m->n > 0 && (!m->ids || !m->scratch)) return ck.bad("NULL ids / scratch");
    if (((uintptr_t)m->ids & 7u) || ((uintptr_t)m->scratch & 7u) || ((uintptr_t)m->state & 15u) || ((uintptr_t)m->overflow & 3u))
        return ck.bad("ids / scratch must be 8-byte aligned, state 16-byte aligned, overflow 4-byte aligned");
    const MctsLayout l = mcts_layout(b->num_envs, m->cap);
    a.n = m->n, a.k = m->k, a.S = m->sim_times, a.max_depth = m->max_depth, a.rollout = m->rollout_length, a.cap = m->cap;
    a.A = A, a.W = b->W, a.L = b->L, a.H = b->H, a.E = b->num_envs;
    a.credit = m->credit, a.zeta = m->zeta;
    a.binvol = (double)b->W * b->L * b->H;
    a.ids = m->ids, a.scratch = m->scratch;
    a.bins = (MBin *)((char *)m->state + l.bins);
    a.mt = (uint32_t *)((char *)m->state + l.mt);
    a.pool = (MRec *)((char *)m->state + l.pool);
    a.overflow = m->overflow;
    a.hmap = b->hmap;
    a.state = b->state;
    return 0;
}

}  // namespace

extern "C" {

int bpp_mcts_sizes(int32_t E, int32_t k, int32_t sim_times, int32_t max_depth, int32_t rollout_length, int32_t W, int32_t L,
                   int64_t out[4]) {
    const ArgCheck ck{"bpp_mcts_sizes"};
    if (!out) return ck.bad("NULL pointer");
    if (E < 0 || W <= 0 || L <= 0 || W * L > kMaxArea) return ck.bad("bad E or geometry");
    if (k < 2 || k > kMctsMaxK) return ck.bad("k must be in 2 .. 16");
    if (sim_times < 1) return ck.bad("sim_times must be positive");
    if (max_depth < 0 || max_depth > k - 1) return ck.bad("max_depth must be in 0 .. k - 1");
    if (rollout_length < -1) return ck.bad("rollout_length must be -1, 0 or positive");
    const int64_t cap = mcts_cap(k, sim_times, max_depth, W * L);
    if (cap > (int64_t)1 << 30) return ck.bad("pool too large");
    const MctsLayout l = mcts_layout(E, cap);
    out[0] = l.total;
    out[1] = cap;
    out[2] = l.per_bin;
    out[3] = mcts_rollout_levels(k, max_depth, rollout_length);
    return 0;
}

int bpp_mcts_seed(const bpp_batch *b, const bpp_mcts *m, const int64_t *ids, const uint32_t *seeds, int32_t count, void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_seed"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (count < 0) return ck.bad("negative count");
    if (count > 0 && (!ids || !seeds)) return ck.bad("NULL pointer");
    if (((uintptr_t)ids & 7u) || ((uintptr_t)seeds & 3u)) return ck.bad("misaligned buffer");
    return launch_items(mcts_seed_kernel, count, stream, a, ids, seeds, count);
}

int bpp_mcts_clear(const bpp_batch *b, const bpp_mcts *m, const int64_t *ids, int32_t count, void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_clear"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (count < 0) return ck.bad("negative count");
    if ((uintptr_t)ids & 7u) return ck.bad("misaligned ids");
    if (!ids) count = a.E;
    return launch_items(mcts_clear_kernel, count, stream, a, ids, count);
}

int bpp_mcts_begin(const bpp_batch *b, const bpp_mcts *m, void *stream) {
    MctsArgs a;
    if (const int rc = mcts_args(b, m, ArgCheck{"bpp_mcts_begin"}, a)) return rc;
    return launch_items(mcts_begin_kernel, a.n, stream, a);
}

int bpp_mcts_select(const bpp_batch *b, const bpp_mcts *m, int32_t level, const uint8_t *step_done, int64_t *actions,
                    void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_select"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (level < 0 || level >= a.max_depth) return ck.bad("level must be in 0 .. max_depth - 1");
    if (level > 0 && a.n > 0 && !step_done) return ck.bad("NULL step_done after level 0");
    if (a.n > 0 && !actions) return ck.bad("NULL actions");
    if ((uintptr_t)actions & 7u) return ck.bad("misaligned actions");
    return launch_slots(mcts_select_kernel, a.n, stream, a, level, step_done, actions);
}

int bpp_mcts_emit(const bpp_batch *b, const bpp_mcts *m, int32_t rollout_level, const uint8_t *step_done, float *obs, void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_emit"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    const int levels = mcts_rollout_levels(a.k, a.max_depth, a.rollout);
    if (rollout_level < 0 || (rollout_level > 0 && rollout_level >= levels)) return ck.bad("rollout_level must be in 0 .. rollout_levels - 1");
    if (a.n > 0 && !obs) return ck.bad("NULL obs");
    if ((uintptr_t)obs & 15u) return ck.bad("obs must be 16-byte aligned");
    return launch_slots(mcts_emit_kernel, a.n, stream, a, rollout_level, step_done, obs);
}

// bpp_mcts_expand and bpp_mcts_rollout take the same arguments under the same checks.
static int mcts_eval_call(const bpp_batch *b, const bpp_mcts *m, const float *value, const float *logits, int64_t *actions,
                          void *stream, bool expand) {
    MctsArgs a;
    const ArgCheck ck{expand ? "bpp_mcts_expand" : "bpp_mcts_rollout"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (a.n > 0 && (!value || !logits || !actions)) return ck.bad("NULL pointer");
    if (((uintptr_t)value & 3u) || ((uintptr_t)logits & 3u) || ((uintptr_t)actions & 7u)) return ck.bad("misaligned buffer");
    return launch_slots(expand ? mcts_expand_kernel : mcts_rollout_kernel, a.n, stream, a, value, logits, actions);
}

int bpp_mcts_expand(const bpp_batch *b, const bpp_mcts *m, const float *value, const float *logits, int64_t *actions, void *stream) {
    return mcts_eval_call(b, m, value, logits, actions, stream, true);
}

int bpp_mcts_rollout(const bpp_batch *b, const bpp_mcts *m, const float *value, const float *logits, int64_t *actions, void *stream) {
    return mcts_eval_call(b, m, value, logits, actions, stream, false);
}

int bpp_mcts_backup(const bpp_batch *b, const bpp_mcts *m, const uint8_t *step_done, void *stream) {
    MctsArgs a;
    if (const int rc = mcts_args(b, m, ArgCheck{"bpp_mcts_backup"}, a)) return rc;
    return launch_items(mcts_backup_kernel, a.n, stream, a, step_done);
}

int bpp_mcts_finish(const bpp_batch *b, const bpp_mcts *m, int64_t *action, int32_t *root_visits, void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_finish"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (a.n > 0 && (!action || !root_visits)) return ck.bad("NULL pointer");
    if (((uintptr_t)action & 7u) || ((uintptr_t)root_visits & 3u)) return ck.bad("misaligned buffer");
    return launch_slots(mcts_finish_kernel, a.n, stream, a, action, root_visits);
}

int bpp_mcts_advance(const bpp_batch *b, const bpp_mcts *m, const uint8_t *done, void *stream) {
    MctsArgs a;
    const ArgCheck ck{"bpp_mcts_advance"};
    if (const int rc = mcts_args(b, m, ck, a)) return rc;
    if (a.n > 0 && !done) return ck.bad("NULL done");
    return launch_slots(mcts_advance_kernel, a.n, stream, a, done);
}

}  // extern "C"
