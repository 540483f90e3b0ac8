/*
 * bpp_multibin.h -- the paper's multi-bin packing (multi_bin/multi_bin.py get_action, driven as its test() drives it) for
 * a batch of pallets: a policy trained on w x w bins places items on a larger W x L pallet by looking at the pallet through
 * sliding w x w windows.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16), next to include/bpp_reorder.h.  Only libbpp_hip.so exports
 * these symbols.  Every pointer is device memory and `stream` a hipStream_t; no call synchronises, and every argument the
 * host can see is checked before any device work (errors: bpp_last_error); ids held in device memory are checked by the
 * kernels (below).
 *
 * Windows.  Window k = kx * Ky + ky (kx outer, ky inner: slipingWindow, multi_bin.py:10-20) covers the pallet cells
 * [dx, dx + w) x [dy, dy + w), dx = kx * s, dy = ky * s, Kx = (W - w) / s + 1, Ky = (L - w) / s + 1, K = Kx * Ky.
 *
 * A decision is a fixed schedule, with the caller's forward between two launches:
 *
 *   bpp_multibin_emit      slot i (pallet ids[i]): K observation rows [4 w^2] (window heights, item x, y, z) and K masks
 *   forward                rows -> value [n K], logits [n K][w^2] (the CNNPro heads of a w x w x H bin)
 *   bpp_multibin_choose    multi_bin.py:28-80: the position in every window, the advantage rule, the pallet action
 *   bpp_step_subset(ids)   (include/bpp_branch.h) or bpp_step when ids[i] = i covers the batch
 *   bpp_multibin_commit    the step's reward becomes the chosen window's last reward (test(), multi_bin.py:91-93)
 *
 * Per pallet the library keeps K window records in `state` (last reward, last value, has-history), zero for a pallet
 * without history.  The history is per episode: commit clears the records of a pallet whose step ended its episode, and
 * bpp_multibin_clear clears listed pallets (a fresh batch: zero-fill `state`).
 *
 * Exactness (float64, no FMA contraction): bin_num = (W L) / (w w); a window with history has
 * adv = bin_num * last_reward + ((double)value - last_value), one without history -0.2; windows are compared in window
 * order with strict >, starting from -1e8.  last_reward is the float64 reward of the step, box_ratio * 10 on success and
 * 0.0 on a failed placement (envs/bpp0/bin3D.py:95-127).
 *
 * No window (every window's mask is all ones, i.e. the item fits nowhere or everywhere in every window): action 0, adv
 * -1e8, window -1, and no value is recorded.  The reference then appends the step's reward to window (0, 0)'s history,
 * and raises KeyError when (0, 0) has none; here the reward is recorded when window 0 has history and dropped otherwise.
 *
 * A slot whose ids[i] lies outside [0, num_envs) touches no pallet and no record: it emits no rows, gets action
 * BPP_ACTION_NOOP, adv 0 and window -1, and its commit does nothing.  Pallets listed twice are a caller error.
 */
#ifndef BPP_MULTIBIN_H
#define BPP_MULTIBIN_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper bound on the windows K of one pallet (a decision scans a pallet's windows one after another). */
#define BPP_MULTIBIN_MAX_K 256

typedef struct bpp_multibin {
    int32_t n;              /* slots                                                                               */
    int32_t w;              /* window side: 1 <= w <= min(W, L), w * w <= 1024                                      */
    int32_t s;              /* stride >= 1                                                                          */
    int32_t K;              /* windows per pallet, as bpp_multibin_sizes gives it                                   */
    const int64_t *ids;     /* [n] pallets of the batch, read only                                                 */
    void *state;            /* bpp_multibin_sizes out[1] bytes, 8-byte aligned: the window records [num_envs][K]     */
    void *work;             /* bpp_multibin_sizes out[2] bytes, 16-byte aligned, any contents: per slot the K masks, the
                               pending window and item of the last emit / choose                                     */
} bpp_multibin;

/* out[0] = K, out[1] = bytes of `state` for E pallets, out[2] = bytes of `work` for n slots.  Errors: w < 1, w > min(W, L),
 * w * w > 1024, s < 1, W * L > 1024, K > BPP_MULTIBIN_MAX_K. */
int bpp_multibin_sizes(int32_t W, int32_t L, int32_t w, int32_t s, int32_t n, int32_t E, int64_t out[3]);

/* obs: [n K][4 w^2] float32, 16-byte aligned: row i K + k is window k of pallet ids[i] under the pallet's current item
 * (the row multi_bin.py:41-47 builds).  The window masks (acktr/utils.py get_possible_position, the "utils" rule of a
 * w x w x H bin, without its all-ones fallback) go to `work`.  Rows of an invalid slot are left as they are. */
int bpp_multibin_emit(const bpp_batch *b, const bpp_multibin *m, float *obs, void *stream);

/* value [n K] and logits [n K][w^2] of the emitted rows -> action int64 [n] (the pallet position lx * L + ly), adv
 * float64 [n] (multi_bin's max_adv) and window int32 [n] (-1: no window).  The position in window k is the first maximum
 * of softmax(logits) (float32) over the cells of its mask: model_loader.evaluate(use_mask=False), then
 * np.argmax(poss * mask).  A window whose mask is all ones (after get_possible_position's fallback) is skipped.  The chosen
 * window's last value becomes value[i K + k]. */
int bpp_multibin_choose(const bpp_batch *b, const bpp_multibin *m, const float *value, const float *logits, int64_t *action,
                        double *adv, int32_t *window, void *stream);

/* step_done: the done output [n] (uint8) of the step of the last choose's actions, row i for slot i. */
int bpp_multibin_commit(const bpp_batch *b, const bpp_multibin *m, const uint8_t *step_done, void *stream);

/* Clear the window records of pallets ids[0 .. n) (ids NULL: every pallet of the batch, n ignored); ids outside
 * [0, num_envs) are skipped. */
int bpp_multibin_clear(const bpp_batch *b, const bpp_multibin *m, const int64_t *ids, int32_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BPP_MULTIBIN_H */
