/*
 * bpp_mcts.h -- the reference's Monte Carlo tree search (MCTS/monteCarlo.py MCTree, MCTS/node.py PutNode, driven as
 * MCTS/mcts_test.py:14-65 drives them) for a batch of bins, with every bin's tree and random stream on the device
 * (DESIGN.md 3.9).
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16), next to include/bpp_reorder.h.  Only libbpp_hip.so exports
 * these symbols.  Every pointer is device memory and `stream` a hipStream_t; no call synchronises, and every argument the
 * host can see is checked before any device work (errors: bpp_last_error); ids held in device memory are checked by the
 * kernels (below).
 *
 * State.  `state` (bpp_mcts_sizes bytes) holds, for EVERY bin e of the batch: a search record, a numpy-legacy MT19937
 * stream (624 words and a position: np.random.seed / randint / choice / random_sample) and a node pool of two halves of
 * `cap` 32-byte records.  A node's children are one block of the pool (a header record holding the node value and the
 * number of children, then one record per child in ascending action: w, p, n, child block, action, terminated, the
 * volume of the item it placed).  bpp_mcts_advance compacts the kept subtree into the other half.  The trees and streams
 * persist across decisions: slot i of a call works on the state of bin ids[i].
 *
 * One decision (slot i searches for real bin ids[i] on scratch bin scratch[i] of the same batch; no rotation):
 *
 *   bpp_mcts_begin                                        plant a root where bin ids[i] has no tree
 *   sim_times times:
 *     bpp_copy_bins(ids -> scratch)                       select()'s copy.deepcopy(sim_env)
 *     level 0 .. max_depth-1: bpp_mcts_select, bpp_step_subset(scratch)     choose_best (commit of the previous step fused)
 *     bpp_mcts_emit                                       commit; observation row of every slot whose leaf is expanded
 *     forward                                             the caller's policy: value [n], logits [n][A]
 *     bpp_mcts_expand                                     children, priors, node value, the first rollout action
 *     rollout level 1 .. rollout_levels-1: bpp_step_subset(scratch), bpp_mcts_emit, forward, bpp_mcts_rollout
 *     bpp_step_subset(scratch) when rollout_levels > 0, bpp_mcts_backup
 *   bpp_mcts_finish                                       MCTree.play + sample_action: action per slot
 *   (the caller steps the real bins)
 *   bpp_mcts_advance(done)                                MCTree.succeed, or a cleared tree where the episode ended
 *
 * rollout_levels (bpp_mcts_sizes out[3]) is the largest box_num of PutNode.roll_out over the depths a leaf can have.  The
 * actions written by select / expand / rollout are BPP_ACTION_NOOP for a slot with nothing to step; the step_done given to
 * emit / backup / the next select is the compact done output of the bpp_step_subset before it (NULL when there was none).
 *
 * A slot whose ids[i] or scratch[i] lies outside [0, num_envs) touches no bin and no state: it never emits a row, its
 * actions are BPP_ACTION_NOOP, and finish gives it action BPP_ACTION_NOOP and 0 visits.  Bins listed twice, or a scratch
 * bin that is also a real bin, are a caller error (MCTSearch.decide(check=True) rejects them).
 */
#ifndef BPP_MCTS_H
#define BPP_MCTS_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BPP_MCTS_MAX_K 16

typedef struct bpp_mcts {
    int32_t n;              /* search slots                                                                          */
    int32_t k;              /* known items, 2 .. BPP_MCTS_MAX_K                                                       */
    int32_t sim_times;      /* simulations per decision, >= 1                                                        */
    int32_t max_depth;      /* min(search_depth, k - 1) (monteCarlo.py:26-29), 0 .. k - 1                             */
    int32_t rollout_length; /* -1, 0 (None or 0: no rollout) or r >= 1 (node.py:105-110)                               */
    int32_t cap;            /* records per pool half, from bpp_mcts_sizes                                            */
    double credit;          /* 0 .. 1 (node.py:101-104)                                                               */
    double zeta;            /* play()'s temperature, > 0                                                              */
    const int64_t *ids;     /* [n] real bins, read only                                                               */
    const int64_t *scratch; /* [n] scratch bins, distinct and disjoint from ids: overwritten by every simulation        */
    void *state;            /* bpp_mcts_sizes bytes, 16-byte aligned, persistent (see above); zero-fill = no trees     */
    int32_t *overflow;      /* [1]: += 1 per slot and decision whose pool half ran out (that slot's search stops)      */
    int32_t reserved;
} bpp_mcts;

/* out[0] = bytes of `state` for a batch of E bins, out[1] = cap: records per pool half, 1 + (max_depth + 1) * sim_times *
 * (W L + 1) (at most (max_depth + 1) * sim_times expanded nodes are alive: the kept subtree's nodes were expanded by the
 * last max_depth decisions, each expansion makes a block of at most W L + 1 records), out[2] = bytes per bin, out[3] =
 * rollout_levels. */
int bpp_mcts_sizes(int32_t E, int32_t k, int32_t sim_times, int32_t max_depth, int32_t rollout_length, int32_t W, int32_t L,
                   int64_t out[4]);

/* np.random.seed(seeds[j]) (init_genrand) for bins ids[j], j < count; the trees are left alone. */
int bpp_mcts_seed(const bpp_batch *b, const bpp_mcts *m, const int64_t *ids, const uint32_t *seeds, int32_t count,
                  void *stream);

/* Drop the trees of bins ids[0..count) (ids NULL: every bin); the random streams continue. */
int bpp_mcts_clear(const bpp_batch *b, const bpp_mcts *m, const int64_t *ids, int32_t count, void *stream);

int bpp_mcts_begin(const bpp_batch *b, const bpp_mcts *m, void *stream);

/* Level `level` (0 .. max_depth - 1) of the descent: actions [n] for bpp_step_subset(scratch). */
int bpp_mcts_select(const bpp_batch *b, const bpp_mcts *m, int32_t level, const uint8_t *step_done, int64_t *actions,
                    void *stream);

/* rollout_level 0: the descent's last level (after the max_depth selects); j >= 1: rollout level j.  obs: [n][4A] float,
 * 16-byte aligned; rows of slots that have nothing to evaluate are left as they are. */
int bpp_mcts_emit(const bpp_batch *b, const bpp_mcts *m, int32_t rollout_level, const uint8_t *step_done, float *obs,
                  void *stream);

/* value [n] (float) and logits [n][A] (float) of the emitted rows: nmodel.evaluate(obs, False), i.e. the float32 softmax
 * of the logits, unmasked.  actions [n]: the first rollout step (BPP_ACTION_NOOP where there is none). */
int bpp_mcts_expand(const bpp_batch *b, const bpp_mcts *m, const float *value, const float *logits, int64_t *actions,
                    void *stream);
int bpp_mcts_rollout(const bpp_batch *b, const bpp_mcts *m, const float *value, const float *logits, int64_t *actions,
                     void *stream);

int bpp_mcts_backup(const bpp_batch *b, const bpp_mcts *m, const uint8_t *step_done, void *stream);

/* action [n] (int64) and the root's visit count [n] (int32). */
int bpp_mcts_finish(const bpp_batch *b, const bpp_mcts *m, int64_t *action, int32_t *root_visits, void *stream);

/* done [n] (uint8): the real step of slot i ended the episode of bin ids[i] (its tree is dropped); otherwise the child of
 * the action finish chose becomes the root (p = 1; n, w, reward and subtree kept). */
int bpp_mcts_advance(const bpp_batch *b, const bpp_mcts *m, const uint8_t *done, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_MCTS_H */
