/*
 * bpp_policy_train.h -- the training pass of the CNNPro trunk: the five 3x3 convolutions and the three 1x1 head
 * convolutions of acktr/model.py:265-323 forward with their activations kept, and backward from the gradient at the head
 * features to the gradient of every trunk weight and bias, float32 on the matrix cores.  The Linear layers of the three heads
 * are not part of it: they stay with the caller.
 *
 * Additive to include/bpp_abi.h and include/bpp_policy.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_POLICY_TRAIN_H
#define BPP_POLICY_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* geom = {S, H, M}, obs / obs_stride and the packed blob `weights` are those of bpp_policy.h; only the first 151 380 floats of
 * the blob (share.0 .. share.8 and the head convolutions) are read.  A = S * S.
 *
 * feat     f32 [n][20 A]: the head features (actor [8][A], mask [8][A], critic [4][A], after their ReLU): exactly the bits
 *          bpp_policy_forward leaves in its workspace -- the same kernel, the same chains in the same order.
 * acts     f32, five dense arrays [n][64][S][S] one behind the other (array l at acts + l * n * 64 A): the post-ReLU output of
 *          share.0, share.2, share.4, share.6, share.8.  This is the src of BPP_KFAC_PATCH (bpp_kfac.h).
 *
 * BPP_E_BADARG, before any device is touched: a NULL pointer, and what bpp_policy_forward refuses of n, geom and obs_stride.
 * The call only enqueues one kernel on `stream`: no host wait, no allocation, capturable into a graph. */
int bpp_policy_trunk_forward_train(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *feat,
                                   float *acts, void *stream);

/* The backward of the above.
 *
 * weights_bwd  f32, bpp_policy_trunk_backward_weights_floats() = 148 736 floats: the trunk's weights packed for the input
 *              gradient, so that the 32 columns a wave loads for one k' are contiguous.  Offsets in floats:
 *
 *                share.2   [k' = oc * 9 + i' * 3 + j'][c] = W[oc][c][2 - i'][2 - j']   [576][64]   at 0
 *                share.4   the same                                                               at 36864
 *                share.6                                                                          at 2 * 36864
 *                share.8                                                                          at 3 * 36864
 *                head convs [h][c] = W_head[h][c], h = 0-7 actor.0, 8-15 mask.0, 16-19 critic.0   [20][64]   at 147456
 *
 *              (share.0 has no input gradient: none is computed with respect to obs.)
 * feat, acts   what bpp_policy_trunk_forward_train wrote for the same obs and weights.
 * grad_feat    f32 [n][20 A]: the gradient at feat.
 * grads        f32, written: five dense arrays [n][64][A] one behind the other, G_1 .. G_5, the gradients at the pre-activation
 *              outputs of share.0 .. share.8 (the src of BPP_KFAC_NCHW), then the masked head gradient gf' [n][20][A].
 * grad_weights f32 [151 380], written: the gradient of the first 151 380 floats of the forward blob in the blob's own layout --
 *              every matrix [k][oc], the gradient of its bias behind it.
 * workspace    bpp_policy_trunk_backward_workspace(geom, n) bytes, 4-byte aligned; workspace_bytes: what the caller holds
 *              there.  Holds nothing between calls.
 *
 * Normative arithmetic.  Everything is float32; nothing is fused except the fmaf chains.
 *   gf'[h][p] = feat[h][p] > 0 ? grad_feat[h][p] : 0.
 *   D_5[c][p] is ONE chain acc = fmaf(gf'[h][p], W_head[h][c], acc) over h = 0 .. 19 from +0; G_5 = acts_5 > 0 ? D_5 : 0.
 *   For l = 5 .. 2: D_{l-1}[c][y][x] is ONE chain over ascending k' = oc * 9 + i' * 3 + j' from +0 of
 *   fmaf(G_l[oc][y + i' - 1][x + j' - 1], W_l[oc][c][2 - i'][2 - j'], acc); a tap outside the image contributes fmaf(0, w, acc);
 *   G_{l-1} = acts_{l-1} > 0 ? D_{l-1} : 0.
 *   This is what v_mfma_f32_32x32x2_f32 computes, two k' per instruction.  Nothing depends on n, on the bin's place in the
 *   batch or on the other bins of its workgroup: a bin's rows of grads are the same bits in any batch.  No gradient image goes
 *   to memory between layers except as the store to grads: the layers go back and forth between two LDS images per bin.
 *
 *   dW_l[k][oc] = sum over rows (b, p) of patch_{l-1}[b, p][k] * G_l[b][oc][p], k = c * 9 + i * 3 + j, the patch of acts_{l-1} (of
 *   obs for share.0: [4][S][S] at obs + b * obs_stride) with zeros outside the image; for the head convolutions the 1x1 case
 *   with acts_5 and gf'.  db_l[oc] is row k = K of the same product on a patch value of 1: the chain fmaf(1, G_l[b][oc][p], acc).
 *   Order: a split is bpp_policy_trunk_backward_info's `bins per split` consecutive bins (a function of geom alone; the last
 *   split may be shorter).  Inside a split every element is ONE chain from +0 over its rows in ascending (b, p).  A second
 *   kernel adds the partials of the splits in ascending split order in double and casts once to float.
 *   No atomic touches a sum: the same bits on every run, on another stream and in a replayed graph.
 *
 * Form.  The input-gradient kernel is the forward trunk kernel's sibling (P bins per workgroup, the same LDS).  The
 * weight-gradient kernel gives a workgroup 64 rows k of one layer ([K + 1][OC] is cut into tiles [ceil((K + 1) / 32)][2]) and one
 * split; per bin it stages the channels its rows touch with their halo, a plane of ones for row K, and G_l [OC][A].
 *
 * BPP_E_BADARG, before any device is touched: a NULL pointer; what bpp_policy_forward refuses of n, geom and obs_stride;
 * workspace_bytes smaller than bpp_policy_trunk_backward_workspace(geom, n); an n whose splits exceed the grid.
 * The call only enqueues three kernels on `stream`: no host wait, no allocation, capturable into a graph. */
int bpp_policy_trunk_backward(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights_bwd, const float *feat,
                              const float *acts, const float *grad_feat, float *grads, float *grad_weights, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Bytes of `workspace`: splits * blocks * 4 tiles * 1024 floats (0 for arguments bpp_policy_trunk_backward refuses). */
size_t bpp_policy_trunk_backward_workspace(const int32_t geom[], int32_t n);

/* Floats of weights_bwd: 148 736 (0 for a geom that is refused). */
size_t bpp_policy_trunk_backward_weights_floats(const int32_t geom[]);

/* The form bpp_policy_trunk_backward takes (documentation and tests; touches no device; BPP_E_BADARG as above or for a NULL out):
 * out = {bins per workgroup of the input-gradient kernel, its LDS bytes, bins per split, splits, the longest chain of the
 * weight gradient in rows (min(n, bins per split) * A), LDS bytes of the weight-gradient kernel, path (1; 0 when refused, which a
 * non-NULL out is told as well), 64-row blocks of all six layers (43)}. */
int bpp_policy_trunk_backward_info(const int32_t geom[], int32_t n, int32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_POLICY_TRAIN_H */
