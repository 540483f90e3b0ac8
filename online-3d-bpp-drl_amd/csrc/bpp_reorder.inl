// bpp_reorder.inl -- the BPP-k reorder search of include/bpp_reorder.h (acktr/reorder.py, unified_test.py:9-27), included
// at the end of bpp_kernels.hip so that the library stays one translation unit.
//
// One wave per search slot.  The tree is wave-uniform work, done by lane 0 on the slot's node pool in global memory with
// float64 values; the lanes do the A-cell work: the observation row (dwordx4 stores), the item masks (update_mask) and the
// softmax / argmax reductions of the position choice.  Lane c owns cells [4c, 4c + 4) + 256 t of every per-cell array it
// touches, so no lane ever reads a cell another lane wrote within a launch.  A slot's record is read by every lane at the
// start of a launch and written back by lane 0 at its end.
namespace {

constexpr int kReorderMaxK = BPP_REORDER_MAX_K;

// A tree node (reorder.py:7-56).  max_v = factorial(height) is recomputed from height.
struct RNode {
    double max_value;     // valid when has_max
    int32_t parent;       // -1: the root
    int32_t first_child;  // -1: not expanded; children are contiguous, in res_idxs order
    int32_t visit;
    int32_t dis_num;
    int32_t action;       // -1: None
    int8_t number, height, nchild, has_max;
};
static_assert(sizeof(RNode) == 32, "RNode layout");

// A slot's search state (128 bytes).
struct RSlot {
    double nor_exp;       // get_baseline's running sum
    double cur_value;     // the descent's running value
    double val;           // value of the last evaluated row
    int32_t nor_act;
    int32_t action;       // the descent's `action` (-1: None)
    int32_t cur_node;
    int32_t next_node;
    int32_t idx;          // item of the emitted row
    int32_t pos;          // position chosen for it
    uint32_t res;         // res_idxs as a bit set
    int32_t nnodes;
    int32_t live;         // the baseline / the current descent goes on
    int32_t pend;         // what the last emit wrote: 0 nothing, 1 a baseline row, 2 a search row
    int32_t wt;           // will_terminate of the emitted row
    int32_t blevel;       // baseline level of the emitted row
    int32_t ovf;          // the node pool ran out
    int32_t ok;           // ids[i] and scratch[i] lie in [0, E): a slot without valid bins never searches
    uint32_t items[kReorderMaxK];   // x | y << 8 | z << 16
    int32_t pad[4];
};
static_assert(sizeof(RSlot) == 128, "RSlot layout");

struct ReorderArgs {
    int32_t n, k, A, W, L, H, max_nodes, mstride;   // mstride: bytes per item mask (A rounded up to 16)
    int32_t E, T, P;
    double binvol, v_bound;
    const int64_t *ids, *scratch;
    RSlot *slots;
    uint8_t *masks;       // [n][k][mstride]
    RNode *nodes;         // [n][max_nodes]
    int32_t *overflow;
    const uint8_t *hmap;
    bpp_env_state *state;
    const uint32_t *pool;
};

__device__ __forceinline__ int32_t factorial_i(int h) {
    int32_t f = 1;
    for (int j = 2; j <= h; ++j) f *= j;
    return f;
}

// Node.get_q_value: the first node upwards that holds a value decides.
__device__ __forceinline__ double node_q(const RNode *nd, int id) {
    while (!nd[id].has_max) id = nd[id].parent;
    const RNode &n = nd[id];
    if (n.visit >= (n.height != -1 ? factorial_i(n.height) : 1)) return -1000.0;
    if (n.dis_num <= 0) return -10000.0;
    return n.max_value;
}

// Node.update, up to the root.
__device__ __forceinline__ void node_update(RNode *nd, int id, double value, int32_t action) {
    for (; id >= 0; id = nd[id].parent) {
        RNode &n = nd[id];
        n.visit += 1;
        if (!n.has_max || value > n.max_value) {
            n.max_value = value;
            n.action = action;
            n.has_max = 1;
        }
    }
}

// Node.disable with the upward dis_num cascade.
__device__ __forceinline__ void node_disable(RNode *nd, int id) {
    for (;;) {
        nd[id].dis_num = 0;
        const int p = nd[id].parent;
        if (p < 0) return;
        nd[p].dis_num -= 1;
        if (nd[p].dis_num != 0) return;
        id = p;
    }
}

__device__ __forceinline__ void init_node(RNode &n, int parent, int number, int height) {
    n.max_value = 0.0;
    n.parent = parent;
    n.first_child = -1;
    n.visit = 0;
    n.dis_num = height;
    n.action = -1;
    n.number = (int8_t)number;
    n.height = (int8_t)height;
    n.nchild = 0;
    n.has_max = 0;
}

// The footprint of item `it` at position `pos` becomes 0 in mask row m (update_mask; numpy slicing clips at the edges).
__device__ __forceinline__ void zero_footprint(const ReorderArgs &a, uint8_t *m, int lane, int pos, uint32_t it) {
    const int px = pos / a.L, py = pos - px * a.L;
    const int x = it & 255, y = (it >> 8) & 255;
    for (int c0 = lane * 4; c0 < a.A; c0 += 4 * kWave)
        for (int c = c0; c < c0 + 4 && c < a.A; ++c) {
            const int cx = c / a.L, cy = c - cx * a.L;
            if (cx >= px && cx < px + x && cy >= py && cy < py + y) m[c] = 0;
        }
}

// Lane 0: the tree part of commit.  Returns 1 when the descent goes on (the caller then zeroes the item's footprint).
__device__ __forceinline__ int commit_search(const ReorderArgs &a, RSlot &s, RNode *nd, bool done, uint32_t item) {
    const int idx = s.idx, k = a.k;
    const int node = s.next_node, cur = s.cur_node;
    if (done || s.wt) {                                          // reorder.py:203-218
        bool fail = false;
        for (int i = 0; i < k; ++i) {
            const bool in = (s.res >> i) & 1u;
            if ((in && i < idx) || (!in && i >= idx)) fail = true;
        }
        if (fail) {
            node_disable(nd, node);
            node_update(nd, cur, -10000.0, -1);
        } else {
            node_update(nd, cur, s.cur_value + 0.0, idx == 0 ? 0 : s.action);
        }
        s.live = 0;
        return 0;
    }
    if (__popc(s.res) == 1) {                                    // reorder.py:220-228: the evaluation point
        node_update(nd, cur, s.cur_value + s.val, idx == 0 ? s.pos : s.action);
        s.live = 0;
        return 0;
    }
    s.res &= ~(1u << idx);                                       // reorder.py:230-242
    s.cur_value = s.cur_value + volume_reward(item_volume(item), a.binvol);
    if (s.action < 0 && idx == 0) s.action = s.pos;
    s.cur_node = node;
    return 1;
}

// Item j of slot i.  The items are written by the begin launch only; they are read from memory because a dynamically
// indexed copy in the slot's registers would live in scratch.
__device__ __forceinline__ uint32_t slot_item(const ReorderArgs &a, int i, int j) { return a.slots[i].items[j]; }

// Commit the step of the row emitted last (s.pend), every lane of the wave.  Lane 0's copy of s is the one kept.
__device__ __forceinline__ void reorder_commit(const ReorderArgs &a, RSlot &s, int i, int lane, const uint8_t *step_done) {
    if (s.pend == 1) {                                           // get_baseline, reorder.py:243-252
        if (lane == 0) {
            const bool done = step_done[i] != 0;
            if (done) s.live = 0;
            else if (s.blevel == a.k - 1) s.nor_exp = s.nor_exp + s.val, s.live = 0;
            else s.nor_exp = s.nor_exp + volume_reward(item_volume(slot_item(a, i, s.blevel)), a.binvol);
        }
    } else if (s.pend == 2) {
        int go = 0;
        if (lane == 0) go = commit_search(a, s, a.nodes + (size_t)i * a.max_nodes, step_done[i] != 0, slot_item(a, i, s.idx));
        go = __shfl(go, 0, kWave);
        if (go) zero_footprint(a, a.masks + ((size_t)i * a.k + s.idx) * a.mstride, lane, s.pos, slot_item(a, i, s.idx));
    }
    if (lane == 0) s.pend = 0;
}

// Lane 0: pick the child of the current node (expanding it first), reorder.py:153-176.  Returns the item, or -1 when the
// descent ends here.
__device__ __forceinline__ int select_child(const ReorderArgs &a, RSlot &s, RNode *nd) {
    RNode &cur = nd[s.cur_node];
    if (cur.first_child < 0) {
        const int cnt = __popc(s.res);
        int made = 0;
        const int first = s.nnodes;
        for (int j = 0; j < a.k; ++j) {
            if (!((s.res >> j) & 1u)) continue;
            if (j == a.k - 1 && cnt > 1) continue;
            if (first + made >= a.max_nodes) {
                if (!s.ovf) atomicAdd(a.overflow, 1);
                s.ovf = 1;
                s.live = 0;
                return -1;
            }
            init_node(nd[first + made], s.cur_node, j, cur.height - 1);
            ++made;
        }
        cur.first_child = first;
        cur.nchild = (int8_t)made;
        s.nnodes = first + made;
    }
    double best = 0.0;
    int pick = -1;
    const double pvisit = sqrt((double)cur.visit);
    for (int c = 0; c < cur.nchild; ++c) {
        const int id = cur.first_child + c;
        const double u = 0.5 * pvisit / (double)(nd[id].visit + 1);
        const double v = node_q(nd, id) + u;                     // get_value
        if (v > best) {
            best = v;
            pick = id;
        }
    }
    if (pick < 0) {
        node_update(nd, s.cur_node, -10000.0, -1);
        s.live = 0;
        return -1;
    }
    s.next_node = pick;
    return nd[pick].number;
}

// bpp_reorder_emit: commit the previous level (step_done), then emit level `level` of iteration `iter` (-1: baseline).
__global__ __launch_bounds__(kWave * kSearchWaves) void reorder_emit_kernel(const ReorderArgs a, int iter, int level,
                                                                              const uint8_t *step_done, float *obs) {
    SEARCH_SLOT_PROLOGUE(a)
    RSlot s = a.slots[i];
    __builtin_amdgcn_wave_barrier();
    if (step_done) reorder_commit(a, s, i, lane, step_done);
    uint8_t *masks = a.masks + (size_t)i * a.k * a.mstride;
    if (iter >= 0 && level == 0) {                               // reorder.py:257-260: a fresh copy, res_idxs and masks
        for (int j = 0; j < a.k; ++j)
            for (int c = lane * 4; c < a.A; c += 4 * kWave) *(uint32_t *)(masks + (size_t)j * a.mstride + c) = 0x01010101u;
        if (lane == 0) {
            RNode *nd = a.nodes + (size_t)i * a.max_nodes;
            if (iter == 0) {                                     // reorder.py:254-256: the root holds the baseline
                nd[0].max_value = s.nor_exp;
                nd[0].action = s.nor_act;
                nd[0].has_max = 1;
            }
            s.cur_node = 0;
            s.res = (1u << a.k) - 1u;
            s.cur_value = 0.0;
            s.action = -1;
            s.live = s.ok && !s.ovf ? 1 : 0;
        }
    }
    int idx = -1;
    if (lane == 0 && s.live) {
        if (iter < 0) idx = level;
        else idx = select_child(a, s, a.nodes + (size_t)i * a.max_nodes);
    }
    idx = __shfl(idx, 0, kWave);
    if (idx < 0) {
        if (lane == 0) a.slots[i] = s;
        return;
    }
    // the observation row: plane 0 mixed with the masks of the items after idx (get_mixed_obs), planes 1-3 the item
    const int64_t sid64 = a.scratch[i];
    if (!bin_in_range(sid64, a.E)) return;                       // (never live: s.ok)
    const int sid = (int)sid64;
    const uint32_t it = slot_item(a, i, idx);
    const float fx = (float)(it & 255u), fy = (float)((it >> 8) & 255u), fz = (float)((it >> 16) & 255u);
    const uint8_t *hm = a.hmap + (size_t)sid * a.A;
    float *row = obs + (size_t)i * 4 * a.A;
    int sum = 0;
    const bool mix = iter >= 0;
    for (int c0 = lane * 4; c0 < a.A; c0 += 4 * kWave) {
        float h[4];
        for (int q = 0; q < 4; ++q) {
            const int c = c0 + q;
            int v = 0;
            if (c < a.A) {
                v = hm[c];
                if (mix)
                    for (int j = idx + 1; j < a.k; ++j)
                        if (masks[(size_t)j * a.mstride + c] == 0) v = a.H;
            }
            h[q] = (float)v;
            sum += v;
        }
        store_obs_quad(row, a.A, c0, h, fx, fy, fz);
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        a.state[sid].item_cur = it;                              // cur_env.box_creator.box_list = [cur_box, ...]
        s.idx = idx;
        s.blevel = level;
        s.wt = mix && sum == a.A * a.H;                          // will_terminate
        s.pend = mix ? 2 : 1;
        a.slots[i] = s;
    }
}

// bpp_reorder_choose: model_loader.evaluate(use_mask=True) and the position rule of the row's phase.
__global__ __launch_bounds__(kWave * kSearchWaves) void reorder_choose_kernel(const ReorderArgs a, const float *value,
                                                                                const float *logits, const float *pred,
                                                                                int64_t *actions) {
    SEARCH_SLOT_PROLOGUE(a)
    RSlot *sp = a.slots + i;
    const int pend = sp->pend;
    if (pend == 0) {
        if (lane == 0) actions[i] = BPP_ACTION_NOOP;
        return;
    }
    const float *lg = logits + (size_t)i * a.A;
    const float *pr = pred ? pred + (size_t)i * a.A : nullptr;
    float mx, sum;
    row_softmax_stats(lg, a.A, lane, mx, sum);
    // the maximum of softmax * binary(pred): baseline np.argmax (first), search argsort[-1] (last)
    const bool last = pend == 2;
    float best = -1.0f;
    int bi = last ? a.A - 1 : 0;                                 // the all-zero rule, also for a row without a number
    for (int c = lane; c < a.A; c += kWave) {
        float p = expf(lg[c] - mx) / sum;
        if (pr && !(pr[c] >= 0.5f)) p = 0.0f;
        if (p > best || (last && p == best)) best = p, bi = c;
    }
    wave_argmax(best, bi, last);
    if (lane == 0) {
        const double v = (double)value[i];
        sp->val = v;
        sp->pos = bi;
        if (pend == 1 && sp->blevel == 0) sp->nor_act = bi;
        actions[i] = bi;
    }
}

__global__ __launch_bounds__(kWave * kSearchWaves) void reorder_begin_kernel(const ReorderArgs a) {
    SEARCH_SLOT_PROLOGUE(a)
    uint8_t *masks = a.masks + (size_t)i * a.k * a.mstride;
    for (int j = 0; j < a.k; ++j)
        for (int c = lane * 4; c < a.A; c += 4 * kWave) *(uint32_t *)(masks + (size_t)j * a.mstride + c) = 0x01010101u;
    if (lane != 0) return;
    RSlot s;
    int id = 0, sid = 0;
    const bool ok = slot_bins(a, i, id, sid);
    const bpp_env_state st = a.state[id];
    for (int j = 0; j < kReorderMaxK; ++j)                       // BoxCreator.preview(k): the terminator repeats past the end
        s.items[j] = j < a.k ? a.pool[(size_t)st.seq * a.T + min(st.cursor + j, a.T - 1)] & 0xFFFFFFu : 0u;
    s.nor_exp = 0.0, s.cur_value = 0.0, s.val = 0.0;
    s.nor_act = -1, s.action = -1, s.cur_node = 0, s.next_node = 0, s.idx = 0, s.pos = 0;
    s.res = (1u << a.k) - 1u;
    s.nnodes = 1;
    s.live = ok ? 1 : 0;
    s.pend = 0, s.wt = 0, s.blevel = 0, s.ovf = 0;
    for (int j = 0; j < 4; ++j) s.pad[j] = 0;
    s.ok = ok ? 1 : 0;
    a.slots[i] = s;
    init_node(a.nodes[(size_t)i * a.max_nodes], -1, -1, a.k - 1);   // Node(None, None, box_num - 1)
}

__global__ __launch_bounds__(kWave * kSearchWaves) void reorder_commit_kernel(const ReorderArgs a, const uint8_t *step_done) {
    SEARCH_SLOT_PROLOGUE(a)
    RSlot s = a.slots[i];
    __builtin_amdgcn_wave_barrier();
    reorder_commit(a, s, i, lane, step_done);
    if (lane == 0) a.slots[i] = s;
}

// reorder_search's last lines (reorder.py:261-270): the conservative rule.  One thread per slot.
__global__ void reorder_finish_kernel(const ReorderArgs a, int64_t *action, double *value, uint8_t *is_default) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.n) return;
    const RSlot *s = a.slots + i;
    if (!s->ok) {                                                // a slot whose ids lie outside [0, E) searched nothing
        action[i] = BPP_ACTION_NOOP;
        value[i] = 0.0;
        is_default[i] = 0;
        return;
    }
    const RNode &root = a.nodes[(size_t)i * a.max_nodes];
    double max_exp = root.max_value;
    int32_t max_act = root.action;
    const double nor_exp = s->nor_exp;
    const int32_t nor_act = s->nor_act;
    if (max_act != nor_act && max_exp - nor_exp < a.v_bound) {
        max_exp = nor_exp;
        max_act = nor_act;
    }
    action[i] = max_act;
    value[i] = max_exp;
    is_default[i] = max_act == nor_act;
}

int64_t reorder_iterations(int k, int times) {
    int64_t f = 1;
    for (int j = 2; j <= k - 1; ++j) f *= j;
    return times < f ? times : f;
}

int64_t reorder_nodes(int k, int64_t iters) {
    int64_t prefixes = 0, p = 1;      // ordered prefixes of the k items: sum_d k! / (k - d)!
    for (int d = 0; d <= k; ++d) {
        prefixes += p;
        p *= k - d;
    }
    const int64_t bound = 1 + iters * k * (k + 1) / 2;
    return bound < prefixes ? bound : prefixes;
}

struct ReorderLayout {
    int64_t slots, masks, nodes, total;
    int32_t mstride;
};

ReorderLayout reorder_layout(int64_t n, int k, int A, int64_t max_nodes) {
    ReorderLayout l;
    l.mstride = (A + 15) / 16 * 16;
    l.slots = 0;
    l.masks = n * (int64_t)sizeof(RSlot);
    l.nodes = l.masks + (n * k * l.mstride + 255) / 256 * 256;
    l.total = l.nodes + n * max_nodes * (int64_t)sizeof(RNode);
    return l;
}

// Everything a reorder call checks before device work; fills the kernel arguments.
int reorder_args(const bpp_batch *b, const bpp_reorder *r, const ArgCheck &ck, ReorderArgs &a) {
    const int rc = check_search_batch(b, r, ck, "the reorder search supports bins without rotation only", true);
    if (rc) return rc;
    if (r->k < 1 || r->k > kReorderMaxK) return ck.bad("k must be in 1 .. 8");
    if (r->n < 0) return ck.bad("negative n");
    if (r->times < 1 || r->times != reorder_iterations(r->k, r->times)) return ck.bad("times must be in 1 .. (k-1)!");
    if (r->max_nodes < 1) return ck.bad("max_nodes must be positive");
    if (r->n > 0 && (!r->ids || !r->scratch || !r->work || !r->overflow)) return ck.bad("NULL pointer");
    if (((uintptr_t)r->ids & 7u) || ((uintptr_t)r->scratch & 7u) || ((uintptr_t)r->work & 15u) || ((uintptr_t)r->overflow & 3u))
        return ck.bad("ids / scratch must be 8-byte aligned, work 16-byte aligned, overflow 4-byte aligned");
    const int A = b->W * b->L;
    const ReorderLayout l = reorder_layout(r->n, r->k, A, r->max_nodes);
    a.n = r->n, a.k = r->k, a.A = A, a.W = b->W, a.L = b->L, a.H = b->H, a.max_nodes = r->max_nodes, a.mstride = l.mstride;
    a.E = b->num_envs, a.T = b->pool_len, a.P = b->pool_size;
    a.binvol = (double)b->W * b->L * b->H;
    a.v_bound = r->v_bound;
    a.ids = r->ids, a.scratch = r->scratch;
    a.slots = (RSlot *)((char *)r->work + l.slots);
    a.masks = (uint8_t *)r->work + l.masks;
    a.nodes = (RNode *)((char *)r->work + l.nodes);
    a.overflow = r->overflow;
    a.hmap = b->hmap;
    a.state = b->state;
    a.pool = (const uint32_t *)b->seq_pool;
    return 0;
}

}  // namespace

extern "C" {

int bpp_reorder_sizes(int32_t n, int32_t k, int32_t times, int32_t W, int32_t L, int64_t out[3]) {
    const ArgCheck ck{"bpp_reorder_sizes"};
    if (!out) return ck.bad("NULL pointer");
    if (n < 0 || W <= 0 || L <= 0 || W * L > kMaxArea) return ck.bad("bad n or geometry");
    if (k < 1 || k > kReorderMaxK) return ck.bad("k must be in 1 .. 8");
    if (times < 1) return ck.bad("times must be positive");
    const int64_t iters = reorder_iterations(k, times);
    const int64_t nodes = reorder_nodes(k, iters);
    out[0] = reorder_layout(n, k, W * L, nodes).total;
    out[1] = iters;
    out[2] = nodes;
    return 0;
}

int bpp_reorder_begin(const bpp_batch *b, const bpp_reorder *r, void *stream) {
    ReorderArgs a;
    if (const int rc = reorder_args(b, r, ArgCheck{"bpp_reorder_begin"}, a)) return rc;
    return launch_slots(reorder_begin_kernel, a.n, stream, a);
}

int bpp_reorder_emit(const bpp_batch *b, const bpp_reorder *r, int32_t iter, int32_t level, const uint8_t *step_done,
                     float *obs, void *stream) {
    ReorderArgs a;
    const ArgCheck ck{"bpp_reorder_emit"};
    if (const int rc = reorder_args(b, r, ck, a)) return rc;
    if (iter < -1 || iter >= r->times || level < 0 || level >= r->k) return ck.bad("iter / level out of range");
    if (a.n > 0 && !obs) return ck.bad("NULL obs");
    if ((uintptr_t)obs & 15u) return ck.bad("obs must be 16-byte aligned");
    return launch_slots(reorder_emit_kernel, a.n, stream, a, iter, level, step_done, obs);
}

int bpp_reorder_choose(const bpp_batch *b, const bpp_reorder *r, const float *value, const float *logits, const float *pred,
                       int64_t *actions, void *stream) {
    ReorderArgs a;
    const ArgCheck ck{"bpp_reorder_choose"};
    if (const int rc = reorder_args(b, r, ck, a)) return rc;
    if (a.n > 0 && (!value || !logits || !actions)) return ck.bad("NULL pointer");
    if (((uintptr_t)value & 3u) || ((uintptr_t)logits & 3u) || ((uintptr_t)pred & 3u) || ((uintptr_t)actions & 7u))
        return ck.bad("misaligned buffer");
    return launch_slots(reorder_choose_kernel, a.n, stream, a, value, logits, pred, actions);
}

int bpp_reorder_commit(const bpp_batch *b, const bpp_reorder *r, const uint8_t *step_done, void *stream) {
    ReorderArgs a;
    const ArgCheck ck{"bpp_reorder_commit"};
    if (const int rc = reorder_args(b, r, ck, a)) return rc;
    if (a.n > 0 && !step_done) return ck.bad("NULL step_done");
    return launch_slots(reorder_commit_kernel, a.n, stream, a, step_done);
}

int bpp_reorder_finish(const bpp_batch *b, const bpp_reorder *r, int64_t *action, double *value, uint8_t *is_default,
                       void *stream) {
    ReorderArgs a;
    const ArgCheck ck{"bpp_reorder_finish"};
    if (const int rc = reorder_args(b, r, ck, a)) return rc;
    if (a.n > 0 && (!action || !value || !is_default)) return ck.bad("NULL pointer");
    if (((uintptr_t)action & 7u) || ((uintptr_t)value & 7u)) return ck.bad("misaligned buffer");
    return launch_items(reorder_finish_kernel, a.n, stream, a, action, value, is_default);
}

}  // extern "C"
