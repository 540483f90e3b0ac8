/*
 * bpp_stream_kinds.h -- the endless device-generated item supply (include/bpp_abi.h: bpp_stream) for the reference's other
 * two item generators: CUT-1 (envs/bpp0/cutCreator.py, `--item-seq cut1`, the reference's default) and RS
 * (envs/bpp0/binCreator.py:24-40, `--item-seq rs`).  bpp_stream_refill cuts CUT-2 sequences; the two refills below fill
 * the same ring, in the same row format, under the same contract, so everything downstream of the ring (the step
 * kernels, the row cache, bpp_copy_bins, checkpoints, the searches) works unchanged.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols (device pointers,
 * `stream` a hipStream_t); the CPU restatement of oracle/ does not.  What the kernels must produce is stated in Python:
 * sequences.cut1_stream_sequence / rs_stream_sequence.
 *
 * bpp_stream is used as it is: sized by bpp_stream_sizes, seeded by bpp_stream_init, rng == BPP_STREAM_RNG_COUNTER only (a
 * bin's record is its 16-byte stream id).  bound_lo / bound_hi only size the `work` scratch there (any pair bpp_stream_sizes
 * accepts: the refills below use the part of `work` the scan kernel writes, which every such pair covers) and do not enter
 * the sequences.
 *
 * Normative definitions (distribution parity with the reference, as for the CUT-2 counter generator).  With
 * R = the counter generator of include/bpp_abi.h keyed by (seed0, the bin's stream id, episode k):
 *
 *   CUT-1  episode k = cutCreator.py:32-128 with every random.choice(list) = list[R.below(len(list))] (also for a list of
 *          one element: the draw index advances), every random.randint(a, b) = a + R.below(b - a + 1), and, with
 *          `rotation`, np.random.rand() = 0.5 * R.below(2) at the place the reference draws it -- the x / y swap of
 *          :119-125 happens exactly when that draw is 1.  Without `rotation` no such draw is made.
 *   RS     item j of episode k = box_set[R.below(n_set)], j = 0, 1, ..., pool_len - 4; the rest of the row is the terminator.
 *          The reference draws without end; a caller keeps rows long enough for a bin to be full before the row ends
 *          (pool_len >= W*L*H / smallest box volume + 3; BppVecEnv refuses shorter rows).
 *
 * Limit of the CUT-1 kernel (one lane per sequence, single-wave workgroups, everything a lane needs in LDS: the piece list
 * with three extents, three offsets and a link per piece, and per piece the supported part of its footprint, which stands in
 * for the W x L support plane of _add_candidate -- so W*L is not limited):
 *   piece bound  W*L*H / (low_x * low_y * low_z) <= BPP_CUT1_MAX_PIECES
 * Anything beyond is refused with BPP_E_BADARG.  So are ranges the reference's own cutter fails on (an assertion in
 * _choose_pos): a bin side below its low, or high < 2 low - 1 on an axis (a piece of low + high .. 2 low - 1 cannot be cut).
 */
#ifndef BPP_STREAM_KINDS_H
#define BPP_STREAM_KINDS_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BPP_STREAM_KIND_CUT1 1
#define BPP_STREAM_KIND_RS 2
#define BPP_CUT1_MAX_PIECES 128
#define BPP_RS_MAX_SET 4096

/* Both refills: same contract as bpp_stream_refill.  Sequences are generated until gen_next[e] == state[e].episode + depth
 * for every bin; rows are written in the ring's format (two look-ahead entries, items, terminator padding; the first two
 * items of a row are repeated in the look-ahead entries of the two rows before); *s->overflow counts the sequences that
 * were cut short (a row too short for the sequence, a box of box_set with a zero side or larger than the bin -- played as
 * the terminator --, a walk that left its bounds).  Arguments are checked before any device is touched; the kernels are only
 * enqueued on `stream`.
 * box_range = (low_x, low_y, low_z, high_x, high_y, high_z), host memory; rotation: 0 / 1, the env's.
 * box_set: DEVICE memory, uint8 [n_set][4] = (x, y, z, 0), 1 <= n_set <= BPP_RS_MAX_SET, 4-byte aligned. */
int bpp_stream_refill_cut1(const bpp_stream *s, const int32_t box_range[6], int32_t rotation, void *stream);
int bpp_stream_refill_rs(const bpp_stream *s, const uint8_t *box_set, int32_t n_set, void *stream);

/* The form a refill of `kind` (BPP_STREAM_KIND_*) takes for this stream: out[0] = sequences (lanes at work) per workgroup,
 * out[1] = bytes of LDS per workgroup, out[2] = pieces a lane's list holds (the geometry's piece bound; 0 for RS), out[3] =
 * threads per workgroup.  box_range as above for CUT-1, ignored for RS.  Pure host function; for documentation and tests. */
int bpp_stream_kinds_info(const bpp_stream *s, int32_t kind, const int32_t box_range[6], int32_t out[4]);

/* bpp_rollout_uniform_stream for a ring of `kind`: nsteps lock-steps under the uniform-feasible policy (the lock-step loop
 * of bpp_rollout_uniform) with the kind's refill on `stream` after every refill_every of them and after the last.  The caller
 * has refilled the ring before the call.  The arguments of the other kind are ignored.  Results equal the same lock-steps
 * taken one by one with a refill every refill_every. */
int bpp_rollout_uniform_stream_kind(const bpp_batch *b, const bpp_step_out *out, int64_t *actions, uint64_t seed, uint64_t step0,
                                    int32_t nsteps, const bpp_stream *s, int32_t refill_every, int32_t kind, const int32_t box_range[6],
                                    int32_t rotation, const uint8_t *box_set, int32_t n_set, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_STREAM_KINDS_H */
