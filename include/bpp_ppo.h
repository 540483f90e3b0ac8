/*
 * bpp_ppo.h -- the native half of a PPO update (acktr/algo/ppo.py:34-95 carried over to the masked head of
 * acktr/distributions.py:71-101): the normalised advantages of a rollout, a row gather for the observations of a mini-batch,
 * and the clipped-surrogate / clipped-value loss of one mini-batch with its gradients at the three network outputs in ONE pass.
 * The storage-side arrays of a mini-batch (feasibility masks, actions, old values, returns, old log-probabilities, advantages)
 * are read IN PLACE through the mini-batch's row indices: no mask row is copied.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.  Every call only
 * enqueues kernels on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph.  No atomic touches a
 * sum: every output is the same bits on every run, on any stream and in a replayed graph.
 */
#ifndef BPP_PPO_H
#define BPP_PPO_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- normalised advantages (ppo.py:34-36) over the E = T * N rows of returns[:-1] and value_preds[:-1] --------------------
 *
 *   returns, value_preds  f32 [E]
 *   adv                   f32 [E], output
 *   stats                 f64 [2], output: mean and unbiased standard deviation of raw
 *   workspace             bpp_ppo_advantages_workspace(E) bytes, 8-byte aligned; holds nothing between calls
 *
 * Normative operations:
 *   raw[i]  = returns[i] - value_preds[i]                                  float32
 *   mean    = SUM_i (double)raw[i] / (double)E                             double
 *   std     = sqrt(SUM_i ((double)raw[i] - mean)^2 / (double)(E - 1))      double; the divisor of torch's .std()
 *   mean_f  = (float)mean,  std_f = (float)std                             each cast once
 *   adv[i]  = (raw[i] - mean_f) / (std_f + 1e-5f)                          float32, unfused
 * Order of both SUMs, from E alone: with C = out[0], G = out[1] and W = out[2] of bpp_ppo_advantages_info, block g owns elements
 * [g C, (g + 1) C); its lane t adds elements g C + t, + W, + 2 W, ... in that order and a binary tree (stride W / 2, ..., 1)
 * adds the W lanes; the G block sums are added the same way by one block: lane t adds sums t, t + W, ..., then the tree.
 *
 * BPP_E_BADARG, before any device is touched: E < 2, a NULL pointer.  Three kernels. */
int bpp_ppo_advantages(const float *returns, const float *value_preds, float *adv, double *stats, int32_t E, void *workspace,
                       void *stream);

/* Bytes of `workspace` for E rows (0 for E < 2). */
size_t bpp_ppo_advantages_workspace(int32_t E);

/* out = {elements per block C, blocks G, lanes per block W}; touches no device; BPP_E_BADARG for E < 2 or a NULL out. */
int bpp_ppo_advantages_info(int32_t E, int32_t out[3]);

/* ---- row gather: dst[b][0 .. len) = src[idx[b]][0 .. len), b < B ------------------------------------------------------------
 *
 *   src   f32, `rows` rows of `src_stride` floats each (src_stride >= len)
 *   idx   i64 [B]
 *   dst   f32 [B][len], dense
 *
 * A wave copies a row, or 512 consecutive floats of a longer one: every load and store instruction of a wave is one contiguous
 * 256-byte segment.  An idx[b] outside [0, rows) reads nothing and makes dst[b] a row of NaN: nothing outside src is read
 * whatever idx holds.  BPP_E_BADARG: B, len or rows < 1, src_stride < len, a NULL pointer.  One kernel. */
int bpp_gather_rows(const float *src, int64_t src_stride, int64_t rows, const int64_t *idx, int32_t B, int32_t len, float *dst,
                    void *stream);

/* ---- the loss of one PPO mini-batch of B rows and its gradients (ppo.py:56-80) --------------------------------------------
 *
 * The network's outputs on the mini-batch, dense:
 *   logits                  f32 [B][M]
 *   values                  f32 [B]
 *   pred_mask               f32 [B][M] or NULL = no mask-prediction term
 * The rollout, E rows, read in place at row r = idx[b]:
 *   idx                     i64 [B] or NULL = the identity (then B <= E)
 *   location_masks          f32 [E][M]
 *   action                  i64 [E]; an action outside [0, M) is treated as bpp_masked_evaluate treats it
 *   value_preds, returns, old_log_probs, adv    f32 [E]
 * Outputs:
 *   grad_logits             f32 [B][M]: d loss / d logits
 *   grad_values             f32 [B]:    d loss / d values
 *   grad_pred_mask          f32 [B][M]: d loss / d pred_mask; not touched when pred_mask is NULL
 *   rows                    f32 [B][7] or NULL: per-row {value term, action term, ent, bad, sq, ratio, clipped}
 *   terms                   f32 [7]: value_loss, action_loss, dist_entropy, prob_loss, graph_loss, loss, clip fraction
 *   workspace               bpp_ppo_loss_workspace(B, M) bytes, 8-byte aligned; holds nothing between calls
 *
 * Normative operations per row b, r = idx[b] -- float32, unfused, in this order.  logp, ent, bad: exactly those of
 * bpp_masked_evaluate on (logits[b], location_masks[r], action[r]).  A = adv[r], old = old_log_probs[r], vp = value_preds[r],
 * R = returns[r], v = values[b].
 *   ratio = expf(logp - old)
 *   lo = (float)(1.0 - clip), hi = (float)(1.0 + clip), c = (float)clip
 *   surr1 = ratio * A,  surr2 = fminf(fmaxf(ratio, lo), hi) * A
 *   action term = -fminf(surr1, surr2)
 *   g_ratio = (surr1 <= surr2) ? A : 0
 *       torch's rule: clamp passes the gradient on the closed interval [lo, hi]; min gives the gradient to the smaller operand and
 *       splits a tie in halves.  surr1 < surr2: all of it through surr1.  A tie inside the interval: both halves reach the ratio,
 *       A in total.  (A tie outside the interval needs A = 0.)  Checked against float64 autograd of the installed torch, at
 *       ratio = 1 with clip = 0.2 (inside) and clip = 0 (both bounds equal the ratio): tests/test_ppo.py.
 *   clipped = (ratio < lo || ratio > hi) ? 1 : 0
 *   d = v - R
 *   use_clipped_value_loss:  t = v - vp,  vpc = vp + fminf(fmaxf(t, -c), c),  e = vpc - R,
 *                            value term = 0.5f * fmaxf(d * d, e * e)
 *                            pass = (t >= -c && t <= c) ? 1 : 0              clamp's closed interval
 *                            g_v = d          when d * d > e * e
 *                                  e * pass   when d * d < e * e
 *                                  0.5f * d + 0.5f * (e * pass)   on a tie   torch's max splits it in halves
 *   otherwise:               value term = 0.5f * (d * d),  g_v = d
 *   sq = as in bpp_a2c_loss (include/bpp_update.h); 0 when pred_mask is NULL
 *   weights, formed in double and cast once to float:
 *       cB    = (float)(1.0 / B)                      c_v   = (float)(value_loss_coef / B)
 *       g_ent = (float)(-entropy_coef / B)            g_bad = (float)(invalid_coef / ((double)B * M))
 *       c_p   = (float)(2.0 * mask_coef / ((double)B * M))
 *   g_logp = -(g_ratio * ratio) * cB
 *   grad_logits[b][:]    = what bpp_masked_evaluate_backward writes for the row under the weights (g_logp, g_ent, g_bad)
 *   grad_values[b]       = c_v * g_v
 *   grad_pred_mask[b][k] = c_p * (pred_mask[b][k] - location_masks[r][k])
 *   the first five terms and the clip fraction = the sums of `rows` columns 0 .. 4 and 6 in DOUBLE, in bpp_a2c_loss's order with
 *       (out[0], out[1], out[3]) of bpp_ppo_loss_info, divided in double by B (prob_loss, graph_loss: by (double)B * M), cast to float
 *   loss = (float)(value_loss_coef * value_loss + action_loss - entropy_coef * dist_entropy + invalid_coef * prob_loss
 *                  + mask_coef * graph_loss), left to right, on the double means.  With both optional coefficients 0 (the defaults
 *                  of bpp_amd.PPO) this is ppo.py:79-80.
 *
 * An idx[b] outside [0, E) reads nothing of the rollout: the row's gradients, its `rows` entries and therefore the terms are NaN.
 *
 * BPP_E_BADARG, before any device is touched: B < 1, E < 1, M < 1, clip < 0 (or NaN), idx NULL with B > E, a NULL logits / values /
 * location_masks / action / value_preds / returns / old_log_probs / adv / grad_logits / grad_values / terms / workspace,
 * pred_mask given without grad_pred_mask.  Two kernels. */
int bpp_ppo_loss(const float *logits, const float *values, const float *pred_mask, const int64_t *idx, const float *location_masks,
                 const int64_t *action, const float *value_preds, const float *returns, const float *old_log_probs, const float *adv,
                 double clip, double value_loss_coef, double entropy_coef, double invalid_coef, double mask_coef,
                 int32_t use_clipped_value_loss, float *grad_logits, float *grad_values, float *grad_pred_mask, float *rows,
                 float *terms, void *workspace, int32_t B, int32_t E, int32_t M, void *stream);

/* Bytes of `workspace` for B rows of M entries (0 for B < 1 or M < 1). */
size_t bpp_ppo_loss_workspace(int32_t B, int32_t M);

/* As bpp_a2c_loss_info, for B rows: out = {rows per workgroup, workgroups of the row kernel, 1 = registers (M <= 512) / 0 = the
 * row is walked in memory, first-level width of the reduction}. */
int bpp_ppo_loss_info(int32_t B, int32_t M, int32_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_PPO_H */
