/*
 * bpp_placements.h -- packing plans recorded on the device: where every box of every bin was placed.
 *
 * The reference keeps the plan as part of Space: self.boxes, a list of Box(x, y, z, lx, ly, lz), and self.flags, the rotation
 * of each (envs/bpp0/space.py:6-16,23-24,176-177); user_study/user_study.py:54-62 writes exactly those six numbers per box.
 * bpp_env_state only counts the boxes.  Here the list is a LOG beside the batch, filled by two small kernels around the step --
 * bpp_placements_note before it, bpp_placements_commit after it -- so the step kernel itself is untouched, and read through
 * bpp_placements_gather.  bpp_placements_replay rebuilds heightmaps from plans and checks every box: the verifier, and what a
 * renderer needs.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols (device pointers,
 * `stream` a hipStream_t); the CPU restatement of oracle/ does not.
 *
 * Every entry point checks its arguments before any device is touched (BPP_E_BADARG, bpp_last_error() = "<function>: <what>"),
 * only enqueues kernels on `stream`, allocates nothing, waits for nothing and can be captured into a graph.
 */
#ifndef BPP_PLACEMENTS_H
#define BPP_PLACEMENTS_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One placed box, 8 bytes.  x, y: the footprint as placed, after the rotation swap (space.py:162-167, "record rotated box");
 * z: the item's height; lz: the height it rests on; cell = lx * L + ly: where its corner is (a side reaches 255 and W * L
 * reaches 1 024, so lx does not fit a byte and the cell index is stored); rotated: space.flags.  Box.standardize() of the
 * record is (x, y, z, cell / L, cell % L, lz). */
typedef struct bpp_placement {
    uint8_t x, y, z, lz;
    uint16_t cell;
    uint8_t rotated, pad;
} bpp_placement;

#define BPP_PLAN_RUNNING  0 /* the episode a bin is playing                 */
#define BPP_PLAN_FINISHED 1 /* the last episode it finished (keep_finished) */
#define BPP_PLACEMENTS_MAX_CAPACITY (1 << 20)

/* The log: opaque, caller-allocated, 16-byte aligned memory of bpp_placements_sizes(E, capacity, keep_finished) bytes (the
 * return value; BPP_E_BADARG for E < 1, capacity outside 1 .. BPP_PLACEMENTS_MAX_CAPACITY).  Per bin it holds `capacity` records
 * of the running episode and their count, with keep_finished != 0 the records, count and episode index of the last FINISHED
 * episode (two banks per bin that change roles when an episode ends: a finished plan is never copied), and an 8-byte note of
 * the lock-step in flight.  Its LAST 8 BYTES are the one shared overflow counter (int32, then padding): records dropped because
 * a plan was longer than `capacity`.  A log belongs to one (E, capacity, keep_finished): pass the same three to every call.
 * Checkpoint it as bytes. */
int64_t bpp_placements_sizes(int32_t E, int32_t capacity, int32_t keep_finished);

/* Every count becomes 0, no finished plan remains, the overflow counter is 0.  Call it once after allocating the log and
 * whenever the bins are reset (bpp_reset): an abandoned episode is not a finished plan. */
int bpp_placements_clear(void *log, int32_t E, int32_t capacity, int32_t keep_finished, void *stream);

/* BEFORE the step, on the same stream.  ids == NULL: all b->num_envs bins with actions[num_envs] (n is not looked at), for
 * bpp_step / bpp_step_dropin; else slot i stands for bin ids[i] with actions[i], n slots, as bpp_step_subset takes them (an id
 * outside [0, num_envs) is skipped).  Per slot: the bin's item on display (bpp_env_state.item_cur) and the action, decoded as the
 * step decodes it -- rotated = b->rotation && a > W * L (the strict comparison of bin3D.py:102), idx = rotated ? a - W * L : a --
 * become the bin's note {x, y after the swap, z, cell = idx, rotated}.  BPP_ACTION_NOOP or an idx outside [0, W * L) leaves an
 * EMPTY note.  Whether the box can be placed is not decided here: that is the step's business. */
int bpp_placements_note(const bpp_batch *b, const int64_t *ids, int32_t n, const int64_t *actions, void *log, int32_t capacity,
                        int32_t keep_finished, void *stream);

/* AFTER the step, on the same stream; ids / n as above, done = the step's bpp_step_out.done ([num_envs], or the compact [n]
 * rows of bpp_step_subset).  An empty note with done == 0 does nothing (the bin was left alone).  done == 0: the note is appended to the bin's running plan with
 * lz = hmap[bin][cell] - z (after update_height_graph, space.py:36-46, the footprint is level at lz + z).  done == 1 -- whatever
 * the note holds: an action outside the bin leaves an empty note and ends the episode like any other failed placement --: the
 * running plan -- without the box that failed -- becomes the bin's finished plan of episode bpp_env_state.episode - 1 (with
 * keep_finished; otherwise it is dropped) and the running count returns to 0.  A record past `capacity` is dropped: the count
 * keeps counting -- it equals bpp_env_state.n_boxes throughout -- and the overflow counter is incremented.  Nothing is ever
 * written outside the log.  The note is consumed. */
int bpp_placements_commit(const bpp_batch *b, const int64_t *ids, int32_t n, const uint8_t *done, void *log, int32_t capacity,
                          int32_t keep_finished, void *stream);

/* The plan side of bpp_copy_bins: the plans (running and finished) and the note of bins dst[i] become those of bins src[i].
 * Same rules: dst distinct and disjoint from src (not checked), a pair with an id outside [0, E) is skipped. */
int bpp_placements_copy(void *log, const int64_t *src, const int64_t *dst, int32_t n, int32_t E, int32_t capacity,
                        int32_t keep_finished, void *stream);

/* Compact rows for bins ids[0..n) (ids == NULL: all E bins, n is not looked at): out_records row i = the `capacity` records
 * of the bin's running (which = BPP_PLAN_RUNNING) or finished (BPP_PLAN_FINISHED; needs keep_finished) plan, rows out_stride >=
 * capacity RECORDS apart, 8-byte aligned; entries from the count on are zero, so the bytes are reproducible.  out_count[i]: boxes
 * of the plan (it may exceed capacity: the rest was dropped), -1 for "no finished episode yet" and for an id outside [0, E).
 * out_episode[i] (may be NULL): the episode index of the plan (running: as of the bin's last recorded box; -1 with the count). */
int bpp_placements_gather(const void *log, const int64_t *ids, int32_t n, int32_t which, void *out_records, int32_t out_stride,
                          int32_t *out_count, int32_t *out_episode, int32_t E, int32_t capacity, int32_t keep_finished, void *stream);

/* The verifier: hmap_out [n][W * L] bytes = the heightmaps of n plans (records rows `stride` >= capacity records apart, count [n]
 * as bpp_placements_gather writes them), built by applying the first min(count, capacity, upto) boxes of each in order (upto < 0:
 * no limit; a negative count: no box); W, L <= 1 024 with W * L <= 1 024, H <= 255.  One wave per plan, the lanes share the cells.  status[i] = -1 when every applied box is
 * sound, else the index of the first that is not -- the heightmap is then the one before that box.  Sound: every side >= 1;
 * lx + x <= W and ly + y <= L; lz equal to the highest cell under the footprint; lz + z <= H.  volume[i]: int32 sum of x * y * z
 * over the applied boxes.  status and volume may be NULL.  Needs no batch: works on plans read back from a file. */
int bpp_placements_replay(const void *records, int32_t stride, int32_t capacity, const int32_t *count, int32_t n, int32_t W,
                          int32_t L, int32_t H, int32_t upto, uint8_t *hmap_out, int32_t *status, int32_t *volume, void *stream);

/* Launch shapes (documentation and tests): out = {lanes per workgroup of note / commit / clear (one lane per bin), their
 * workgroups for E bins, waves per workgroup of copy / gather / replay (one wave per bin or plan), their workgroups for E, cells
 * per lane of replay (the power of two that covers A / 64), bytes of a record}. */
int bpp_placements_info(int32_t E, int32_t capacity, int32_t A, int32_t out[6]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_PLACEMENTS_H */
