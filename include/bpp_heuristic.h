/*
 * bpp_heuristic.h -- the lowest-top packing heuristic on the device: per bin, among the entries its mask offers,
 * the placement whose resulting top is lowest, then the one that leaves the smoothest surface, then the lowest index.  The baseline
 * packer of the package: what a checkpoint is compared with, what fills bins to realistic depth, what a run is warm-started from.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.  bpp_heuristic_act only
 * enqueues one kernel on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph.  All of it is integer
 * arithmetic; no atomic, one writer per output: a bin's result depends on nothing but the bin's own row -- the same bits in any
 * batch, on any stream and in a replayed graph.
 */
#ifndef BPP_HEURISTIC_H
#define BPP_HEURISTIC_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `rule` */
#define BPP_HEUR_LOWEST_TOP 0       /* lowest top, then smoothest surface, then lowest index (the default) */
#define BPP_HEUR_LOWEST_TOP_PLAIN 1 /* lowest top, then lowest index */

/* ---- the rule, per bin; A = W * L, M = A * (1 + rotation) -----------------------------------------------------------------
 *
 *   obs    f32, n rows of `obs_stride` floats (obs_stride >= 4 A): plane 0 the heightmap, planes 1 .. 3 the item's x, y, z
 *          broadcast -- the observation row of bpp_step, as bpp_policy_forward takes it (storage slots, column slices)
 *   mask   f32 [n][M], dense
 *   action i64 [n], output
 *   top    i32 [n] or NULL, output: `best` below where it is < INF, else -1
 *
 * Normative operations:
 *   h[i][j] = rint(obs[i L + j]), i < W, j < L;  (x, y, z) = rint(obs[A]), rint(obs[2 A]), rint(obs[3 A])
 *   entry m is ON iff mask[m] > 0.5
 *   entry m decodes as  half = (m >= A),  pos = m - half A,  (i, j) = divmod(pos, L),  footprint (fx, fy) = (x, y) for half 0
 *       and (y, x) for half 1.  (`>= A`, not the environment's strict `> A`: index A is scored as the rotated footprint at
 *       (0, 0).  The environment decodes it un-rotated and may fail it; a caller that offers it in the mask gets it scored.)
 *   m is IN RANGE iff 1 <= fx <= W, 1 <= fy <= L, i + fx <= W, j + fy <= L;  then
 *       top(m) = max(h over the fx x fy window at (i, j)) + z
 *   key K(m) = top(m) if m is on and in range;  INF if m is on and not in range;  INF + 1 if m is off
 *   best = min K
 *   BPP_HEUR_LOWEST_TOP_PLAIN: action = the lowest m with K(m) = best.  (A mask that is all off gives 0; an all-ones fallback
 *       mask whose entries are all out of range gives the lowest on entry.)
 *   BPP_HEUR_LOWEST_TOP: the same, unless best < INF and more than one m has K(m) = best.  Then, for each such m, h' = h with
 *       the window's cells set to `best`, inside a border one cell wide all round that is also at `best`;
 *       R(m) = the sum of |h'(a) - h'(b)| over all 4-neighbour pairs of the padded (W + 2) x (L + 2) map;
 *       action = the lowest m with the smallest R.
 * Only the action (and `top`) is normative, not the way to it: the kernel scores a tied entry by R(m) minus the bin's constant
 * R(h), which only the edges that touch the window contribute to.
 *
 * Contract inputs: integer-valued heights in [0, 255], sides in [0, 255], W * L <= 1024 (bpp_limits).  For ANY float input --
 * NaN, infinities, sides of 1e9, whatever lies in the padding of a wider row -- the kernel reads nothing outside the n rows of obs
 * and mask, writes nothing but action[n] and top[n], terminates, and gives an action in [0, M): every value is clamped before it
 * is converted (heights and z to [0, 255], x and y to [0, 256]; NaN takes the lower bound), a side outside [1, W] / [1, L] makes
 * its whole half out of range, and every loop is bounded by M or by the window.
 *
 * BPP_E_BADARG, before any device is touched: a NULL obs, mask or action; n <= 0; W or L < 1; a geometry past bpp_limits;
 * rotation not 0 or 1; an unknown rule; obs_stride < 4 A.  One kernel. */
int bpp_heuristic_act(const float *obs, int64_t obs_stride, const float *mask, int32_t n, int32_t W, int32_t L, int32_t rotation,
                      int32_t rule, int64_t *action, int32_t *top /* may be NULL */, void *stream);

/* out = {bins per wave, LDS bytes per workgroup, workgroups, path}; path 0: 16 lanes per bin, four bins per wave (A <= 128),
 * path 1: one bin per wave.  A workgroup is four waves.  Touches no device; BPP_E_BADARG as above, and for a NULL out. */
int bpp_heuristic_act_info(int32_t W, int32_t L, int32_t rotation, int32_t n, int32_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_HEURISTIC_H */
