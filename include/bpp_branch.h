/*
 * bpp_branch.h -- native branch stepping for lookahead searches: step, observe and clone a SUBSET of a batch's bins
 * (SURVEY.md 8f row f4).  The reference's searches work on copy.deepcopy(env) branches (acktr/reorder.py:181-262,
 * MCTS/node.py:92-137); here the branches are bins of one bpp_batch, and these calls cost what the listed bins cost,
 * whatever the batch size.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these two symbols (device
 * pointers, `stream` a hipStream_t); the CPU restatement of oracle/ does not, and the tests check them against
 * bpp_step with BPP_ACTION_NOOP for the other bins and against a copy of the bin records.
 */
#ifndef BPP_BRANCH_H
#define BPP_BRANCH_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Step bins ids[0..n) with actions[0..n): slot i performs for bin ids[i] exactly what bpp_step performs for it (placement
 * rule, heightmap, reward, Monitor sums, auto-reset, ep_acc row ids[i], next observation and mask; with out->next_action
 * the fused uniform draw, hashed with the bin's global id env_id_base + ids[i]) and writes ROW i of the compact [n]-row
 * buffers of `out` (obs [n][4A], mask [n][M], reward / done / counter / ratio / ep_ret / ep_len [n], next_action [n],
 * host_reward / host_done [n]).  No other bin is read or written.  BPP_ACTION_NOOP re-emits a bin's observation and mask
 * without stepping it.
 * An id outside [0, num_envs) touches no bin: its row holds the outputs of a no-op of an empty bin -- reward 0, done 0,
 * counter / ratio / ep_ret / ep_len 0, zero observation and mask, next_action 0 -- and, with bad_ids != NULL (int32 [1],
 * device memory), bumps *bad_ids.  Duplicate ids are a caller error: the slots race on that bin's state (never on memory
 * outside the buffers).  ids and actions: int64 [n], 8-byte aligned; n == 0 is a no-op. */
int bpp_step_subset(const bpp_batch *b, const int64_t *ids, int32_t n, const int64_t *actions, const bpp_step_out *out,
                    int32_t *bad_ids, void *stream);

/* Bins dst[i] become copies of bins src[i] (copy.deepcopy(env) of the searches), one launch for all pairs: byte heightmap
 * row and the 48-byte state record.  With a ring pool (b->pool_mode == BPP_POOL_RING; `s` is the ring's bpp_stream, NULL
 * for a static pool) the copy continues the SOURCE's item stream: the bin's `depth` ring rows, its generator record and
 * gen_next are copied too and bpp_env_state.seq is rebased by dst - src (a ring row number encodes the bin).  The row
 * cache lines of the dst bins are dropped, those of no other bin.  Nothing is re-emitted: call bpp_step_subset with
 * BPP_ACTION_NOOP on dst for their observations.  A pair with an id outside [0, num_envs) is skipped.  The pairs are
 * copied concurrently: dst must be distinct and disjoint from src (not checked here). */
int bpp_copy_bins(const bpp_batch *b, const bpp_stream *s, const int64_t *src, const int64_t *dst, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_BRANCH_H */
