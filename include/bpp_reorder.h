/*
 * bpp_reorder.h -- the BPP-k reorder search (acktr/reorder.py ReorderTree, driven as unified_test.py:9-27 drives it) for a
 * batch of bins, with every bin's search tree kept on the device.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16), next to include/bpp_branch.h, whose calls it is driven with.
 * Only libbpp_hip.so exports these symbols.  Every pointer is device memory and `stream` a hipStream_t; no call
 * synchronises, and every argument the host can see is checked before any device work (errors: bpp_last_error); ids
 * held in device memory are checked by the kernels (below).
 *
 * Slot i searches for real bin ids[i] on scratch bin scratch[i] of the same batch (no rotation, static pool).  One decision
 * is a FIXED schedule of launches, whatever each slot's tree does:
 *
 *   bpp_reorder_begin                                                  previews the k items, plants the root
 *   bpp_copy_bins(ids -> scratch)                                      the baseline's copy.deepcopy(env)
 *   k times:      bpp_reorder_emit, forward, bpp_reorder_choose, bpp_step_subset(scratch)       get_baseline
 *   times times:  bpp_copy_bins(ids -> scratch), then k times the same four                     search()
 *   bpp_reorder_commit, bpp_reorder_finish
 *
 * bpp_reorder_emit(step_done != NULL) first COMMITS the step before it (update / disable / backup, item masks, running
 * value), then emits the next level: per slot it picks the child, writes item_cur of the scratch bin and observation row i
 * [4A] (plane 0 raised to H where a later item's mask is zero: get_mixed_obs).  The caller's forward maps the rows to
 * value / logits / pred, bpp_reorder_choose turns them into a position per slot (BPP_ACTION_NOOP for a slot whose
 * descent has ended), and bpp_step_subset steps the scratch bins with those actions.
 *
 * A slot whose ids[i] or scratch[i] lies outside [0, num_envs) touches no bin: it never emits a row, its actions are
 * BPP_ACTION_NOOP, and bpp_reorder_finish gives it action BPP_ACTION_NOOP, value 0 and is_default 0.  Bins listed twice
 * are a caller error (ReorderSearch.decide(check=True) rejects them).
 */
#ifndef BPP_REORDER_H
#define BPP_REORDER_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BPP_REORDER_MAX_K 8

typedef struct bpp_reorder {
    int32_t n;              /* search slots                                                                          */
    int32_t k;              /* previewed items, 1 .. BPP_REORDER_MAX_K                                                */
    int32_t times;          /* search iterations: min(times, (k-1)!) (acktr/reorder.py:75), from bpp_reorder_sizes     */
    int32_t max_nodes;      /* tree nodes per slot, from bpp_reorder_sizes                                            */
    double v_bound;         /* the conservative rule's threshold (reorder.py:259)                                     */
    const int64_t *ids;     /* [n] real bins, read only                                                               */
    const int64_t *scratch; /* [n] scratch bins, distinct and disjoint from ids: overwritten by every iteration         */
    void *work;             /* bpp_reorder_sizes bytes, 16-byte aligned, any contents: slots, item masks, node pools   */
    int32_t *overflow;      /* [1]: += 1 per slot whose node pool ran out (its search stops; never with the sizes given) */
    int32_t reserved;
} bpp_reorder;

/* out[0] = bytes of `work`, out[1] = the search iterations min(times, (k-1)!), out[2] = nodes per slot: 1 + iterations *
 * k (k + 1) / 2 (a descent expands at most one node per level, a node at depth d gets at most k - d children), capped by
 * the number of ordered item prefixes. */
int bpp_reorder_sizes(int32_t n, int32_t k, int32_t times, int32_t W, int32_t L, int64_t out[3]);

/* Preview the k items of every real bin (BoxCreator.preview(k)), plant the root, start the baseline. */
int bpp_reorder_begin(const bpp_batch *b, const bpp_reorder *r, void *stream);

/* iter = -1: baseline level `level`; iter >= 0: level `level` of search iteration iter.  step_done: the compact done
 * output [n] of the bpp_step_subset of the previous level (its commit is fused in front), NULL before the first level.
 * obs: [n][4A] float, 16-byte aligned; rows of slots that have nothing to evaluate are left as they are. */
int bpp_reorder_emit(const bpp_batch *b, const bpp_reorder *r, int32_t iter, int32_t level, const uint8_t *step_done,
                     float *obs, void *stream);

/* value [n], logits [n][A] and pred [n][A] (NULL: every position allowed) of the emitted rows -> actions [n] for
 * bpp_step_subset: model_loader.evaluate(use_mask=True) (softmax(logits) * (pred >= 0.5), float32), then np.argmax in the
 * baseline (first maximum) and argsort(...)[-1] in the search (last maximum; an all-zero row gives A - 1, which is what
 * numpy 2.x sorts to the end for A <= 256).  BPP_ACTION_NOOP for a slot without an emitted row. */
int bpp_reorder_choose(const bpp_batch *b, const bpp_reorder *r, const float *value, const float *logits, const float *pred,
                       int64_t *actions, void *stream);

/* Commit the last level's step (step_done as for bpp_reorder_emit). */
int bpp_reorder_commit(const bpp_batch *b, const bpp_reorder *r, const uint8_t *step_done, void *stream);

/* reorder_search's result per slot: action [n] (int64), value [n] (float64: max_exp), is_default [n] (uint8). */
int bpp_reorder_finish(const bpp_batch *b, const bpp_reorder *r, int64_t *action, double *value, uint8_t *is_default,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_REORDER_H */
