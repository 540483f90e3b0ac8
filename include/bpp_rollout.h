/*
 * bpp_rollout.h -- returns of a rollout held on the device: the four variants of the reference's
 * RolloutStorage.compute_returns (acktr/storage.py:72-111) as ONE launch.
 *
 * The recurrences are independent per bin and sequential in t: a lane owns a bin (or four adjacent ones) and walks t from
 * T - 1 down to 0 in registers.  bpp_compute_returns_host runs the same per-bin function on host pointers: the explicit
 * twin for a storage that lives on the CPU, and what the CPU suite checks against the reference bit for bit.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_ROLLOUT_H
#define BPP_ROLLOUT_H

#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N bins, T time steps, every array row-major [rows][N].
 *
 *   rewards      f32 [T][N]
 *   value_preds  f32 [T+1][N]; use_gae: row T is overwritten with next_value (storage.py:80,98)
 *   next_value   f32 [N]
 *   done         u8  [T][N] or NULL.  Non-NULL: the mask of step t + 1 is done[t] ? 0.f : 1.f -- what the step kernel wrote
 *                (bpp_step_out.done), no float conversion pass -- and it is also stored to masks[t + 1].  NULL: `masks` is read.
 *   masks        f32 [T+1][N]: input when done is NULL, else rows 1 .. T are outputs (may then be NULL: not stored).  Row 0 is
 *                never touched.
 *   bad_masks    f32 [T+1][N] or NULL = a row of ones; the arithmetic is carried out all the same (x * 1 + (1 - 1) * v), so
 *                that -0.0 behaves as in the reference.
 *   returns      f32 [T+1][N], output.  use_gae: rows 0 .. T-1 only; otherwise all T + 1 rows, row T = next_value.
 *   advantages   f32 [T][N] or NULL: returns[t] - value_preds[t], computed when the row is final.
 *   gamma, gae_lambda  doubles, as Python passes them.
 *
 * Normative operations -- float32, unfused, in this order; g = (float)gamma, gl = (float)(gamma * gae_lambda) with the product
 * taken in double; m and bad are the values of row t + 1:
 *   use_gae:        delta = (rewards[t] + (g * value_preds[t+1]) * m) - value_preds[t]
 *                   gae   = delta + (gl * m) * gae                  (gae = 0.f before t = T - 1)
 *                   gae   = gae * bad                               (use_proper_time_limits only)
 *                   returns[t] = gae + value_preds[t]
 *   else, proper:   returns[t] = (((returns[t+1] * g) * m) + rewards[t]) * bad + (1.f - bad) * value_preds[t]
 *   else:           returns[t] = ((returns[t+1] * g) * m) + rewards[t]
 *
 * BPP_E_BADARG, before any device is touched: T < 1, N < 1, a NULL rewards / value_preds / next_value / returns, both done
 * and masks NULL.  The device entry point only enqueues one kernel on `stream` (a hipStream_t): no host wait, no allocation,
 * capturable into a graph.  16-byte accesses are used when N % 4 == 0 and every array starts 16-byte aligned (done: 4-byte);
 * any other N or alignment takes the one-bin-per-lane path.  Same bits either way. */
int bpp_compute_returns(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                        const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                        int32_t use_proper_time_limits, double gamma, double gae_lambda, void *stream);
int bpp_compute_returns_host(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                             const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                             int32_t use_proper_time_limits, double gamma, double gae_lambda);


/* Which form bpp_compute_returns takes for these arguments (documentation and tests; touches no device, same argument checks):
 * out = {bins per lane: 4 = 16-byte accesses, 1 = one bin per lane; lanes per workgroup; workgroups}. */
int bpp_compute_returns_info(const float *rewards, float *value_preds, const float *next_value, const uint8_t *done, float *masks,
                             const float *bad_masks, float *returns, float *advantages, int32_t T, int32_t N, int32_t use_gae,
                             int32_t use_proper_time_limits, double gamma, double gae_lambda, int32_t out[3]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_ROLLOUT_H */
