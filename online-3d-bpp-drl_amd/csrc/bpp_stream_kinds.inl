// bpp_stream_kinds.inl -- the ring refills of the reference's other two item generators, CUT-1 and RS
// (include/bpp_stream_kinds.h), their host entry points and the rollout driver that runs them between the lock-steps.
// Included by bpp_kernels.hip behind bpp_drivers.inl.
//
// Both refills are the rows pipeline of bpp_stream_gen.inl with another algorithm in the lane: the scan kernel lists the
// ring rows to rewrite (bin | episode << 32) and the episode every bin is brought to, then ONE LANE PER ROW generates the
// row's sequence from CtrRng::key(seed0, the bin's stream id, episode) -- a pure function of the three, so rows are
// independent of each other -- and writes it in the ring's format: items behind the two look-ahead entries, terminator
// padding, the first two items into the look-ahead entries of the two rows before (place_lookahead).  Neither generator
// sorts, so there is no staging and no sort kernel.  Single-wave workgroups, no communication between lanes.
//
// The statements the kernels are checked against, draw for draw: sequences.cut1_stream_sequence / rs_stream_sequence.

namespace {

constexpr int kKindLanes = 64;          // threads of a workgroup: one wave
constexpr int kKindLdsMost = 64 * 1024; // LDS of a workgroup; a geometry whose 64 lanes need more puts fewer lanes to work
constexpr uint32_t kNil = 255u;         // end of a piece list (BPP_CUT1_MAX_PIECES < 255)
static_assert(BPP_CUT1_MAX_PIECES < 255, "a link is a byte and 255 ends a list");

// A CUT-1 piece: extents d = x | y << 8 | z << 16, offsets o likewise, and the link to the piece behind it in its list.  (Bytes
// in one word, not arrays: the axis of a cut is data, and a register array indexed by data lives in scratch memory.)
struct Piece {
    uint32_t d, o, next;
};
__device__ __forceinline__ uint32_t axis_of(uint32_t packed, uint32_t k) { return (packed >> (8u * k)) & 255u; }
__device__ __forceinline__ uint32_t bytes_to_nibbles(uint32_t v) { return (v & 15u) | ((v >> 4) & 0xf0u) | ((v >> 8) & 0xf00u); }
__device__ __forceinline__ uint32_t nibbles_to_bytes(uint32_t v) { return (v & 15u) | ((v & 0xf0u) << 4) | ((v & 0xf00u) << 8); }
// A lane's pieces in LDS, entry w of the lane at word w * st (st = lanes at work in the workgroup): one word per piece where
// every extent and offset is below 16 (FB = 4: extents in bits 0-11, offsets in bits 12-23, four bits each, next << 24), else two
// (FB = 8: d | next << 24, then o).
template <int FB>
struct PieceCol {
    uint32_t *p;        // &words[lane]
    uint32_t st;
    __device__ __forceinline__ Piece get(uint32_t i) const {
        if constexpr (FB == 4) {
            const uint32_t v = p[i * st];
            return Piece{nibbles_to_bytes(v & 0xfffu), nibbles_to_bytes((v >> 12) & 0xfffu), v >> 24};
        } else {
            const uint32_t a = p[2 * i * st];
            return Piece{a & 0x00ffffffu, p[(2 * i + 1) * st], a >> 24};
        }
    }
    __device__ __forceinline__ void set(uint32_t i, const Piece &c) const {
        if constexpr (FB == 4) {
            p[i * st] = bytes_to_nibbles(c.d) | (bytes_to_nibbles(c.o) << 12) | (c.next << 24);
        } else {
            p[2 * i * st] = c.d | (c.next << 24);
            p[(2 * i + 1) * st] = c.o;
        }
    }
    __device__ __forceinline__ void set_next(uint32_t i, uint32_t next) const {
        uint32_t &w = p[(FB == 4 ? i : 2 * i) * st];
        w = (w & 0x00ffffffu) | (next << 24);
    }
};

struct Cut1Args {
    uint32_t low, high;     // low_x | low_y << 8 | low_z << 16, high likewise
    int32_t rotation;
    int32_t pieces;         // entries of a lane's piece list: the geometry's piece bound
    int32_t lanes;          // lanes at work per workgroup
};

__host__ __device__ inline int cut1_piece_words(int fb) { return fb == 4 ? 1 : 2; }
// per piece the supported part of its footprint: a byte where sides are below 16 (an area of at most 225), else 16 bits
__host__ __device__ inline int cut1_cover_bits(int fb) { return fb == 4 ? 8 : 16; }
__host__ __device__ inline int cut1_cover_words(int pieces, int fb) { return (pieces * cut1_cover_bits(fb) + 31) / 32; }
// bytes of LDS per lane: the piece list, then the supported parts
__host__ __device__ inline size_t cut1_lane_bytes(int pieces, int fb) {
    return (size_t)(pieces * cut1_piece_words(fb) + cut1_cover_words(pieces, fb)) * 4;
}

// One CUT-1 sequence into `row` (TI entries behind the look-ahead header; at most TI - 1 items, the last entry stays the
// terminator).  Returns the number of items written; `over` is set when the sequence was cut short.  cutCreator.py by line:
//   :78-95  _cut_box: passes over the piece list until every piece is inside the range; a piece outside it is replaced, in
//           place, by its two parts (_choose_pos, :58-76: random.choice over the axes out of range, random.randint for the
//           position).  Here the list is linked: the first part takes the piece's entry, the second a new entry linked
//           behind it -- the order of the reference's rebuilt list without moving anything.
//   :97-106 _add_candidate: pieces whose footprint of the plane stands exactly at their base move, in list order, to the
//           end of the candidate list (the same link byte: a piece is in one list at a time).  There is no plane here: the
//           pieces partition the bin and a piece is only placed on complete support, so a cell of the plane stands at a
//           piece's base exactly when the piece right below that cell (its top is that base) has been placed, or the base is
//           the floor.  A piece is therefore supported once the placed pieces whose top is its base cover its whole
//           footprint: every placement adds its overlap to the pieces resting on it, and the piece whose sum reaches its
//           area is a candidate -- in the same call of _add_candidate in which the reference's comparison first holds.
//   :111-128 generate_box_size: random.randint picks a candidate, the coin swaps x / y (rotation only), the plane rises.
// Every loop is bounded by the list capacity: a pass without a cut ends the cutting, a cut takes a new entry, and an
// entry is popped once.
template <int FB>
__device__ __forceinline__ int cut1_generate(CtrRng &rng, const PieceCol<FB> col, uint32_t *cover, int W, int L, int H, const Cut1Args &a,
                                             uint32_t *row, int TI, bool &over) {
    const uint32_t cap = (uint32_t)a.pieces;
    uint32_t n = 1, head = 0;
    col.set(0u, Piece{(uint32_t)W | ((uint32_t)L << 8) | ((uint32_t)H << 16), 0u, kNil});
    for (uint32_t pass = 0, again = 1; again && pass <= cap; ++pass) {
        again = 0;
        uint32_t i = head;
        for (uint32_t visits = 0; i != kNil && visits < cap; ++visits) {
            Piece b = col.get(i);
            uint32_t m = 0;                     // bit k: axis k is outside its range
            for (uint32_t k = 0; k < 3; ++k) m |= (uint32_t)(axis_of(b.d, k) < axis_of(a.low, k) || axis_of(b.d, k) > axis_of(a.high, k)) << k;
            if (m == 0) {
                i = b.next;
                continue;
            }
            const uint32_t pick = rng.below((uint32_t)__popc(m));                       // random.choice(df_list), :66: the pick-th axis set
            const uint32_t m1 = m & (m - 1u);
            const uint32_t df = pick == 0u ? (uint32_t)__ffs((int)m) - 1u : (pick == 1u ? (uint32_t)__ffs((int)m1) - 1u : 2u);
            const int lo = (int)axis_of(a.low, df), hi = (int)axis_of(b.d, df) - lo;
            if (hi < lo || n >= cap) {                                                  // (the reference asserts) / list full
                over = true;
                return 0;
            }
            const uint32_t pos = (uint32_t)lo + rng.below((uint32_t)(hi - lo + 1));     // random.randint(lo, hi), :75
            Piece c2 = b;                       // the part beyond the cut; b becomes the part before it
            c2.d = b.d - (pos << (8u * df));
            c2.o = b.o + (pos << (8u * df));
            b.d = (b.d & ~(255u << (8u * df))) | (pos << (8u * df));
            b.next = n;
            col.set(i, b);
            col.set(n, c2);
            ++n;
            again = 1;
            i = c2.next;
        }
    }
    const uint32_t st = col.st;
    for (uint32_t k = 0; k < (uint32_t)cut1_cover_words(a.pieces, FB); ++k) cover[k * st] = 0u;
    constexpr uint32_t CB = FB == 4 ? 8u : 16u, CPW = 32u / CB, CM = (1u << CB) - 1u;     // bits of a sum, sums per word
    uint32_t chead = kNil, ctail = kNil, ncand = 0;
    // `placed`: the piece that has just been put down, NULL for the first call (nothing placed: the floor supports).
    const auto add_candidates = [&](const Piece *placed) {
        const uint32_t level = placed ? (placed->o >> 16) + (placed->d >> 16) : 0u;
        const uint32_t px = placed ? placed->o & 255u : 0u, py = placed ? (placed->o >> 8) & 255u : 0u;
        const uint32_t pw = placed ? placed->d & 255u : 0u, pl = placed ? (placed->d >> 8) & 255u : 0u;
        uint32_t prev = kNil, i = head;
        for (uint32_t visits = 0; i != kNil && visits < cap; ++visits) {
            const Piece b = col.get(i);
            const uint32_t bx = b.o & 255u, by = (b.o >> 8) & 255u, bw = b.d & 255u, bl = (b.d >> 8) & 255u;
            bool ok = (b.o >> 16) == level;
            if (ok && placed) {
                const uint32_t x0 = max(bx, px), x1 = min(bx + bw, px + pw), y0 = max(by, py), y1 = min(by + bl, py + pl);
                ok = x0 < x1 && y0 < y1;
                if (ok) {
                    uint32_t &w = cover[(i / CPW) * st];
                    const uint32_t sh = (i % CPW) * CB, got = ((w >> sh) & CM) + (x1 - x0) * (y1 - y0);
                    w = (w & ~(CM << sh)) | (got << sh);
                    ok = got == bw * bl;
                }
            }
            if (ok) {
                if (prev == kNil) head = b.next;
                else col.set_next(prev, b.next);
                col.set_next(i, kNil);
                if (ctail == kNil) chead = i;
                else col.set_next(ctail, i);
                ctail = i;
                ++ncand;
            } else {
                prev = i;
            }
            i = b.next;
        }
    };
    add_candidates(nullptr);
    int nv = 0;
    for (uint32_t items = 0; ncand && items < cap; ++items) {
        uint32_t k = rng.below(ncand), prev = kNil, i = chead;                          // cands.pop(random.randint(0, len - 1))
        for (; k && i != kNil; --k) prev = i, i = col.get(i).next;
        if (i == kNil) {
            over = true;
            break;
        }
        const Piece b = col.get(i);
        if (prev == kNil) chead = b.next;
        else col.set_next(prev, b.next);
        if (ctail == i) ctail = prev;
        --ncand;
        const bool swap = a.rotation && rng.below(2u) == 1u;                            // np.random.rand() >= 0.5, :119
        const uint32_t item = swap ? ((b.d >> 8) & 255u) | ((b.d & 255u) << 8) | (b.d & 0x00ff0000u) : b.d;
        if (nv < TI - 1) row[nv++] = item;
        else over = true;
        add_candidates(&b);
    }
    if (head != kNil || ncand) over = true;     // pieces left behind: the walk left its bounds
    return nv;
}

// What both kernels do with a finished row: terminator padding, look-ahead copies, the overflow count.
__device__ __forceinline__ void kind_finish_row(const bpp_stream &s, int bin, int ep, uint32_t *row, int nv, bool over) {
    const int TI = s.pool_len - kRowHdr;
    const uint32_t term = stream_terminator(s);
    for (int k = nv; k < TI; ++k) row[k] = term;
    place_lookahead(s, bin, ep, nv > 0 ? row[0] : term, nv > 1 ? row[1] : term);
    if (over && s.overflow) atomicAdd(s.overflow, 1);
}

// The row a lane serves in round q0 of the scan's list: false for a lane without one.  The lane that writes a bin's newest row
// moves the bin's gen_next (as stream_cut_rows_kernel does).
__device__ __forceinline__ bool kind_row_of_lane(const bpp_stream &s, const StreamWork &w, int q, int &bin, int &ep, uint64_t &sid) {
    if (q >= w.hdr[3]) return false;
    const int64_t id = w.rows[q];
    bin = (int)(uint32_t)id, ep = (int)(id >> 32);
    sid = ctr_stream_id(s, bin);
    if (ep + 1 == w.target[bin]) s.gen_next[bin] = ep + 1;
    return true;
}

template <int FB>
__global__ __launch_bounds__(kKindLanes) void stream_cut1_rows_kernel(bpp_stream s, StreamWork w, Cut1Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    if (lane >= a.lanes) return;            // no workgroup-level synchronisation below
    uint32_t *words = (uint32_t *)smem;
    const PieceCol<FB> col{words + lane, (uint32_t)a.lanes};
    uint32_t *cover = words + (size_t)a.pieces * cut1_piece_words(FB) * a.lanes + lane;
    const int TI = s.pool_len - kRowHdr;
    const int nrows = w.hdr[3];
    for (int q0 = (int)blockIdx.x * a.lanes; q0 < nrows; q0 += (int)gridDim.x * a.lanes) {
        int bin, ep;
        uint64_t sid;
        if (!kind_row_of_lane(s, w, q0 + lane, bin, ep, sid)) continue;
        uint32_t *row = ring_row(s, ep, bin) + kRowHdr;
        CtrRng rng = CtrRng::key(s.seed0, sid, (uint32_t)ep);
        bool over = false;
        const int nv = cut1_generate<FB>(rng, col, cover, s.W, s.L, s.H, a, row, TI, over);
        kind_finish_row(s, bin, ep, row, nv, over);
    }
}

__global__ __launch_bounds__(kKindLanes) void stream_rs_rows_kernel(bpp_stream s, StreamWork w, const uint8_t *box_set, int32_t n_set) {
    const int lane = threadIdx.x;
    const int TI = s.pool_len - kRowHdr;
    const int nrows = w.hdr[3];
    const uint32_t *set = (const uint32_t *)box_set;
    for (int q0 = (int)blockIdx.x * kKindLanes; q0 < nrows; q0 += (int)gridDim.x * kKindLanes) {
        int bin, ep;
        uint64_t sid;
        if (!kind_row_of_lane(s, w, q0 + lane, bin, ep, sid)) continue;
        uint32_t *row = ring_row(s, ep, bin) + kRowHdr;
        CtrRng rng = CtrRng::key(s.seed0, sid, (uint32_t)ep);
        bool over = false;
        for (int k = 0; k < TI - 1; ++k) {                                              // binCreator.py:35-37, one draw per item
            const uint32_t v = set[rng.below((uint32_t)n_set)] & 0x00ffffffu;
            const uint32_t x = v & 255u, y = (v >> 8) & 255u, z = v >> 16;
            const bool fits = x && y && z && z <= (uint32_t)s.H &&
                              ((x <= (uint32_t)s.W && y <= (uint32_t)s.L) || (x <= (uint32_t)s.L && y <= (uint32_t)s.W));
            over = over || !fits;
            row[k] = fits ? v : stream_terminator(s);
        }
        kind_finish_row(s, bin, ep, row, TI - 1, over);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
struct Cut1Plan {
    Cut1Args a;
    int fb;
    size_t lds;
};

int check_kind_stream(const ArgCheck &ck, const bpp_stream *s) {
    if (!s) return ck.bad("NULL pointer");
    if (s->rng != BPP_STREAM_RNG_COUNTER) return ck.bad("needs rng == BPP_STREAM_RNG_COUNTER");
    if (check_stream(s)) {          // (its message names bpp_stream: put this call's name in front)
        char inner[sizeof g_err];
        snprintf(inner, sizeof inner, "%s", g_err);
        return ck.bad(inner);
    }
    return 0;
}

// The geometry and range checks of CUT-1 and the form its kernel takes (no pointer of `s` is looked at).
int plan_cut1(const ArgCheck &ck, const bpp_stream *s, const int32_t box_range[6], int32_t rotation, Cut1Plan &p) {
    if (!box_range) return ck.bad("NULL pointer");
    if (s->W < 1 || s->L < 1 || s->H < 1 || s->W > 255 || s->L > 255 || s->H > 255) return ck.bad("bin sides must be in 1 .. 255");
    const int side[3] = {s->W, s->L, s->H};
    int64_t vol = 1;
    for (int k = 0; k < 3; ++k) {
        const int lo = box_range[k], hi = box_range[3 + k];
        if (lo < 1 || lo > hi) return ck.bad("box_range needs 1 <= low <= high on every axis");
        if (side[k] < lo) return ck.bad("a bin side is below its low: the reference's cutter cannot cut this bin");
        if (hi < 2 * lo - 1) return ck.bad("box_range needs high >= 2 low - 1 on every axis (else a piece can be too long to keep and too short to cut)");
        p.a.low |= (uint32_t)lo << (8 * k), p.a.high |= (uint32_t)(hi < 255 ? hi : 255) << (8 * k);
        vol *= lo;
    }
    const int64_t pieces = (int64_t)s->W * s->L * s->H / vol;
    if (pieces > BPP_CUT1_MAX_PIECES) return ck.bad("more than BPP_CUT1_MAX_PIECES = 128 pieces possible (W*L*H / (low_x*low_y*low_z))");
    if (s->pool_len - 1 - kRowHdr < 1) return ck.bad("pool_len too small");
    p.a.rotation = rotation ? 1 : 0;
    p.a.pieces = (int32_t)pieces;
    p.fb = stream_field_bits(s->W, s->L, s->H);
    const size_t lane_bytes = cut1_lane_bytes(p.a.pieces, p.fb);
    p.a.lanes = kKindLanes;
    while ((size_t)p.a.lanes * lane_bytes > (size_t)kKindLdsMost) p.a.lanes /= 2;        // 64 * 1 280 bytes at the cap with two-word pieces: 32 lanes
    p.lds = lane_bytes * p.a.lanes;
    return 0;
}

// The scan both refills start with: which rows to rewrite, which episode every bin is brought to (always `depth` rows).
int kind_scan(const bpp_stream *s, hipStream_t st, StreamWork &w) {
    const StreamPlan p = plan_stream(s);
    unsigned char *base = (unsigned char *)s->work;
    w = StreamWork{(int32_t *)base, (int32_t *)(base + p.off_jobs), (int32_t *)(base + p.off_target), (int64_t *)(base + p.off_rows),
                   (uint32_t *)(base + p.off_spill), (uint32_t *)(base + p.off_twist), p.cap, p.nsp, p.nslots, p.maxn, p.fb, 0, 0, p.stage};
    const hipError_t e = hipMemsetAsync(base, 0, 64, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    const int E = s->num_envs;
    hipLaunchKernelGGL(stream_scan_kernel, dim3((E + kScanThreads - 1) / kScanThreads), dim3(kScanThreads), 2 * (kScanThreads / 64) * 4 * sizeof(int), st,
                       *s, w);
    return launched();
}

unsigned kind_grid(const bpp_stream *s, int lanes) {
    const int64_t waves = ((int64_t)s->num_envs * s->depth + lanes - 1) / lanes;
    return (unsigned)(waves < 8192 ? waves : 8192);
}

int check_rs(const ArgCheck &ck, const uint8_t *box_set, int32_t n_set) {
    if (!box_set) return ck.bad("NULL pointer");
    if (n_set < 1 || n_set > BPP_RS_MAX_SET) return ck.bad("box_set needs 1 .. BPP_RS_MAX_SET = 4096 boxes");
    if ((uintptr_t)box_set & 3u) return ck.bad("misaligned box_set");
    return 0;
}

int refill_cut1(const ArgCheck &ck, const bpp_stream *s, const int32_t box_range[6], int32_t rotation, void *stream) {
    int rc = check_kind_stream(ck, s);
    if (rc) return rc;
    Cut1Plan p{};
    rc = plan_cut1(ck, s, box_range, rotation, p);
    if (rc) return rc;
    StreamWork w;
    rc = kind_scan(s, (hipStream_t)stream, w);
    if (rc) return rc;
    with_field_bits(p.fb, [&](auto fb) {
        constexpr int FB = decltype(fb)::value;
        hipLaunchKernelGGL(stream_cut1_rows_kernel<FB>, dim3(kind_grid(s, p.a.lanes)), dim3(kKindLanes), p.lds, (hipStream_t)stream, *s, w, p.a);
    });
    return launched();
}

int refill_rs(const ArgCheck &ck, const bpp_stream *s, const uint8_t *box_set, int32_t n_set, void *stream) {
    int rc = check_kind_stream(ck, s);
    if (rc == 0) rc = check_rs(ck, box_set, n_set);
    if (rc) return rc;
    StreamWork w;
    rc = kind_scan(s, (hipStream_t)stream, w);
    if (rc) return rc;
    hipLaunchKernelGGL(stream_rs_rows_kernel, dim3(kind_grid(s, kKindLanes)), dim3(kKindLanes), 0, (hipStream_t)stream, *s, w, box_set, n_set);
    return launched();
}

}  // namespace

extern "C" {

int bpp_stream_refill_cut1(const bpp_stream *s, const int32_t box_range[6], int32_t rotation, void *stream) {
    return refill_cut1(ArgCheck{"bpp_stream_refill_cut1"}, s, box_range, rotation, stream);
}

int bpp_stream_refill_rs(const bpp_stream *s, const uint8_t *box_set, int32_t n_set, void *stream) {
    return refill_rs(ArgCheck{"bpp_stream_refill_rs"}, s, box_set, n_set, stream);
}

int bpp_stream_kinds_info(const bpp_stream *s, int32_t kind, const int32_t box_range[6], int32_t out[4]) {
    const ArgCheck ck{"bpp_stream_kinds_info"};
    if (!s || !out) return ck.bad("NULL pointer");
    if (kind == BPP_STREAM_KIND_RS) {
        out[0] = kKindLanes, out[1] = 0, out[2] = 0, out[3] = kKindLanes;
        return 0;
    }
    if (kind != BPP_STREAM_KIND_CUT1) return ck.bad("unknown kind");
    Cut1Plan p{};
    const int rc = plan_cut1(ck, s, box_range, 0, p);
    if (rc) return rc;
    out[0] = p.a.lanes, out[1] = (int32_t)p.lds, out[2] = p.a.pieces, out[3] = kKindLanes;
    return 0;
}

int bpp_rollout_uniform_stream_kind(const bpp_batch *b, const bpp_step_out *out, int64_t *actions, uint64_t seed, uint64_t step0,
                                    int32_t nsteps, const bpp_stream *s, int32_t refill_every, int32_t kind, const int32_t box_range[6],
                                    int32_t rotation, const uint8_t *box_set, int32_t n_set, void *stream) {
    const ArgCheck ck{"bpp_rollout_uniform_stream_kind"};
    if (!b || !s || !out || !out->mask || !actions) return ck.bad("NULL pointer");
    if (nsteps < 0) return ck.bad("negative nsteps");
    if (kind != BPP_STREAM_KIND_CUT1 && kind != BPP_STREAM_KIND_RS) return ck.bad("unknown kind");
    const int behind = b->seq_cache ? 4 : 3;   // rows a step launch may touch from the current one on (bpp_rollout_uniform_stream)
    if (b->pool_mode != BPP_POOL_RING || refill_every < 1 || refill_every > s->depth - behind)
        return ck.bad("needs a ring pool and 1 <= refill_every <= depth - 3 (- 4 with seq_cache)");
    int rc = check_kind_stream(ck, s);          // what the refills would refuse, before the first lock-step is enqueued
    Cut1Plan probe{};
    if (rc == 0) rc = kind == BPP_STREAM_KIND_CUT1 ? plan_cut1(ck, s, box_range, rotation, probe) : check_rs(ck, box_set, n_set);
    if (rc) return rc;
    const auto refill = [&]() {
        return kind == BPP_STREAM_KIND_CUT1 ? refill_cut1(ck, s, box_range, rotation, stream) : refill_rs(ck, s, box_set, n_set, stream);
    };
    const RolloutGroup g{b, nullptr, out, actions, out->mask, stream};
    int32_t chunk = 0;
    for (int32_t done = 0; rc == 0 && done < nsteps; done += refill_every, ++chunk) {
        const int32_t n = nsteps - done < refill_every ? nsteps - done : refill_every;
        // as in bpp_rollout_uniform_stream: only the first chunk draws its first action with a launch of its own
        rc = rollout_lock_steps(&g, 1, 1, seed, step0 + (uint64_t)done, n, chunk == 0, done + n < nsteps, 0);
        if (rc == 0) rc = refill();
    }
    return rc;
}

}  // extern "C"
