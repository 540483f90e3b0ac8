/*
 * bpp_pipeline.h -- the pipelined rollout driver: the bins of one batch split into G groups, every group's chain of
 * step-kernel launches on a stream of its own ("Pipelined rollout driver").
 *
 * Bins are independent: lock-step t + 1 of a group needs lock-step t of that group only.  On ONE stream launch t + 1 of the
 * whole batch waits until the last workgroup of launch t has retired -- the chip drains, idles for the launch gap and fills
 * again, once per lock-step.  With G chains the workgroups of another group take the slots a finishing launch frees.  A group
 * is what a multi-GPU rank's shard already is (num_envs, env_id_base and offset pointers): item sequences, draws and ep_acc
 * rows are keyed by GLOBAL bin id, so every result is bit-identical to the single-chain driver's.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols (device pointers,
 * `stream` a hipStream_t); the CPU restatement of oracle/ has no streams to split a batch over.
 */
#ifndef BPP_PIPELINE_H
#define BPP_PIPELINE_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BPP_PIPELINE_MAX_GROUPS 4    /* a process opens four hardware queues by default: one per chain, none shared */
#define BPP_PIPELINE_ALIGN      64   /* group boundaries are multiples of this many bins: the most bins one workgroup of the
                                        tile step kernel owns in any launch shape (4 waves x 4 bins x 4 groups per wave), so no
                                        workgroup's bins are split; every per-bin array then starts 64-byte aligned as well */
#define BPP_PIPELINE_MIN_GROUP  8192 /* smallest group bpp_pipeline_plan makes.  One resident round of the tile step kernel is
                                        2 048 workgroups (256 CUs x 8) = 8 192 bins in its smallest launch shape (4 waves x 1 bin,
                                        20x20 bins); a chain of launches below one round leaves slots empty whatever runs beside it */

/* The streams and events the pipelined driver needs beside the caller's stream: max_groups - 1 non-blocking streams, one fork
 * event and one join event per side stream, on the calling thread's CURRENT device.  Created and owned by the caller (one per
 * env, like bpp_side_create); the library keeps no per-device state.  1 <= max_groups <= BPP_PIPELINE_MAX_GROUPS, else
 * BPP_E_BADARG (checked before any device is touched).  bpp_pipeline_destroy waits for the side streams, then releases them;
 * NULL is a no-op.  One pipe serves one call at a time: two host threads must not drive the same pipe concurrently. */
int bpp_pipeline_create(void **pipe, int32_t max_groups);
int bpp_pipeline_destroy(void *pipe);

/* Pure host function: split bins [0, E) into at most `groups` contiguous, disjoint ranges first[g] .. first[g] + count[g]
 * that cover [0, E) in order.  Every boundary is a multiple of BPP_PIPELINE_ALIGN; every group holds at least
 * BPP_PIPELINE_MIN_GROUP bins, so fewer groups come back when E is small (E < 2 * BPP_PIPELINE_MIN_GROUP: one).  The groups
 * are as equal as the alignment allows; the LAST one takes the remainder and may be ragged.  groups == 1 returns the whole
 * range.  `first` and `count` hold `groups` entries.  Returns the number of groups made (>= 1), or BPP_E_BADARG
 * (E <= 0, groups outside 1 .. BPP_PIPELINE_MAX_GROUPS, NULL). */
int bpp_pipeline_plan(int32_t E, int32_t groups, int32_t *first, int32_t *count);

/* bpp_rollout_uniform_sets (include/bpp_abi.h) with the batch split by bpp_pipeline_plan(b->num_envs, groups): the same
 * arguments, the same semantics, bit-identical results in every buffer.  Group g steps bins first[g] .. of `b` as a batch of
 * its own -- num_envs = count[g], env_id_base + first[g], hmap / state / ep_acc, every non-NULL array of every output set,
 * first_mask and actions offset by first[g] rows -- so a launch of one group reads and writes no byte of another.
 *
 * Ordering: group 0 runs on `stream`, group g > 0 on the pipe's stream g - 1.
 *   fork  an event recorded on `stream` at entry; every side stream waits for it, so all groups see whatever was enqueued on
 *         `stream` before the call (reset, an earlier rollout, the caller's own kernels);
 *   join  an event recorded on each side stream behind its last launch; `stream` waits for all of them before the call returns,
 *         so events recorded on `stream` around the call bracket ALL the work, and anything enqueued on `stream` afterwards sees
 *         every group finished.
 * Nothing is captured into a graph and the host never waits.  The launches are enqueued INTERLEAVED -- lock-step t of every
 * group, then lock-step t + 1 -- so that every queue has work from the first microsecond (chain by chain, the second chain
 * would start only after the host had enqueued all of the first).
 * A group's launches have the shape a batch of the group's size gets (bpp_launch_info(count[g], ...)).
 *
 * Refused with BPP_E_BADARG: a BPP_POOL_RING batch (ring rows are indexed by LOCAL bin and num_envs), a seq_cache, output
 * sets with host_reward / host_done, groups outside 1 .. BPP_PIPELINE_MAX_GROUPS, and -- when the plan yields more than one
 * group -- a NULL pipe, more groups than the pipe was created for, a pipe created on another device than the current one.
 * When the plan yields one group (groups == 1, or a batch too small to split) the call IS bpp_rollout_uniform_sets on
 * `stream`; `pipe` may then be NULL. */
int bpp_rollout_uniform_sets_pipelined(const bpp_batch *b, const bpp_step_out *outs, int32_t nsets, const float *first_mask,
                                       int64_t *actions, uint64_t seed, uint64_t step0, int32_t nsteps, int32_t flags,
                                       void *pipe, int32_t groups, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_PIPELINE_H */
