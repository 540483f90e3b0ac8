/*
 * bpp_update.h -- the loss of the A2C update and its gradients as ONE pass over the data: the five terms of the
 * reference's update (acktr/algo/acktr_pipeline.py:45-92: value loss, action loss, entropy, invalid-probability loss and
 * mask-prediction loss), their weighted total, and the gradients of that total with respect to the three network outputs
 * (logits, values, predicted mask).  Every coefficient of the total is known before the backward pass starts, so the
 * gradients need no second visit: one wave per row reads logits, location mask and predicted mask once and writes the two
 * gradient arrays once.  The acktr=False path of the reference (K-FAC: include/bpp_kfac.h).
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_UPDATE_H
#define BPP_UPDATE_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* E rows (T * N of a rollout), M actions per row, every array row-major and dense.
 *
 *   logits, location_masks  f32 [E][M]
 *   action                  i64 [E]; an action outside [0, M) is treated as bpp_masked_evaluate treats it
 *   values, returns         f32 [E]
 *   pred_mask               f32 [E][M] or NULL = no mask-prediction term
 *   grad_logits             f32 [E][M], output: d loss / d logits
 *   grad_values             f32 [E],    output: d loss / d values (the action loss takes the advantage detached)
 *   grad_pred_mask          f32 [E][M], output: d loss / d pred_mask; not touched when pred_mask is NULL
 *   rows                    f32 [E][5] or NULL: per-row {adv * adv, -(adv * logp), ent, bad, sq}
 *   terms                   f32 [6], output: value_loss, action_loss, dist_entropy, prob_loss, graph_loss, loss
 *   workspace               bpp_a2c_loss_workspace(E, M) bytes, 8-byte aligned; holds nothing between calls
 *
 * Normative operations -- float32, unfused, in this order.  logp, ent, bad: exactly those of bpp_masked_evaluate.
 *   adv  = returns[e] - values[e]
 *   sq   = sum_k (pred_mask[k] - mask[k])^2: lane l of the row's wave adds its entries k = l, l + 64, ... in that order, the 64
 *          partial sums go through the wave's butterfly (as every row sum of bpp_masked_evaluate); 0 when pred_mask is NULL
 *   weights, formed in double and cast once to float:
 *          cE    = (float)(1.0 / E)                       cEM = (float)(1.0 / ((double)E * M))
 *          g_ent = (float)(-entropy_coef / E)             g_bad = (float)(invalid_coef / ((double)E * M))
 *          c_v   = (float)(-2.0 * value_loss_coef / E)    c_p   = (float)(2.0 * mask_coef / ((double)E * M))
 *   g_logp = -(adv * cE)
 *   grad_logits[e][:]    = what bpp_masked_evaluate_backward writes for the row under the weights (g_logp, g_ent, g_bad)
 *   grad_values[e]       = c_v * adv
 *   grad_pred_mask[e][k] = c_p * (pred_mask[k] - mask[k])
 *   the five terms       = the sums of the five `rows` columns in DOUBLE, in an order that depends on E alone (below), divided in
 *                          double by E (prob_loss and graph_loss: by (double)E * M) and cast to float
 *   loss = (float)(value_loss_coef * value_loss + action_loss + invalid_coef * prob_loss - entropy_coef * dist_entropy
 *                  + mask_coef * graph_loss), left to right, on the double means
 *
 * Order of the sums: with R = out[0] and G = out[1] of bpp_a2c_loss_info, workgroup g owns rows [g R, (g + 1) R); its wave w
 * adds rows g R + w, + 4, + 8, ... in that order, the workgroup's partial is ((w0 + w1) + w2) + w3; lane t of ONE final
 * workgroup of out[3] lanes adds partials t, t + out[3], ... and a binary tree (stride out[3] / 2, ..., 1) adds the lanes.  No
 * atomic touches a sum: the terms are the same bits on every run.
 *
 * BPP_E_BADARG, before any device is touched: E < 1, M < 1, a NULL logits / location_masks / action / values / returns /
 * grad_logits / grad_values / terms / workspace, pred_mask given without grad_pred_mask.  The call only enqueues two kernels
 * on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph. */
int bpp_a2c_loss(const float *logits, const float *location_masks, const int64_t *action, const float *values, const float *returns,
                 const float *pred_mask, double value_loss_coef, double entropy_coef, double invalid_coef, double mask_coef,
                 float *grad_logits, float *grad_values, float *grad_pred_mask, float *rows, float *terms, void *workspace, int32_t E,
                 int32_t M, void *stream);

/* Bytes of `workspace` for E rows of M entries (0 for E < 1 or M < 1). */
size_t bpp_a2c_loss_workspace(int32_t E, int32_t M);

/* The form bpp_a2c_loss takes for E rows of M entries (documentation and tests; touches no device, BPP_E_BADARG for E < 1,
 * M < 1 or a NULL out): out = {rows per workgroup, workgroups of the row kernel, 1 = a lane holds its entries of the row in
 * registers (M <= 512) / 0 = it walks the row in memory, first-level width of the reduction}.  Same bits either way. */
int bpp_a2c_loss_info(int32_t E, int32_t M, int32_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_UPDATE_H */
