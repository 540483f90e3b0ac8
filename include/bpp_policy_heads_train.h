/*
 * bpp_policy_heads_train.h -- the training pass of the six Linear layers of CNNPro's three heads: actor.3 and
 * dist.linear, mask.3 and mask.5, critic.3 and critic_linear of acktr/model.py:265-323 and acktr/distributions.py:72, forward
 * with the hidden vectors kept, and backward from the gradients at value, logits and pred to the gradient at the head features
 * and to the gradient of every Linear weight and bias, float32 on the matrix cores.  With include/bpp_policy_train.h the whole
 * network trains natively: this call's grad_feat is that header's grad_feat.
 *
 * Additive to include/bpp_abi.h and include/bpp_policy.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_POLICY_HEADS_TRAIN_H
#define BPP_POLICY_HEADS_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* geom = {S, H, M} and the packed blob `weights` are those of bpp_policy.h; the heads read the blob from float 151 380 on.
 * A = S * S.  Head order everywhere: actor (logits), mask (pred), critic (value).  K1 = 8 A, 8 A, 4 A input features of a head
 * at f0 = 0, 8 A, 16 A of a row of feat; Mh = M, M, 1 outputs.
 *
 * feat     f32 [n][20 A]: what bpp_policy_trunk_forward_train wrote (or bpp_policy_forward left in its workspace).
 * value    f32 [n], logits f32 [n][M], pred f32 [n][M], written: bit for bit what bpp_policy_forward gives for the same feat and
 *          blob -- the same kernel with one more store, the same chains in the same order.
 * hidden   f32 [3][n][H], written: the post-ReLU output of actor.3, mask.3, critic.3; row b of head h dense at
 *          hidden + (h * n + b) * H.  These are BPP_KFAC_ROWS sources (bpp_kfac.h), as the slices of feat are.
 *
 * BPP_E_BADARG, before any device is touched: a NULL pointer; what bpp_policy_forward_one_image refuses of n and geom (S <= 22, H
 * a multiple of 32 up to 512, M = A or 2 A, n >= 1).  The heads hold no LDS image, so sides up to 22 are accepted although the
 * trunk's training pass stops at 15.
 * The call only enqueues one kernel on `stream`: no host wait, no allocation, capturable into a graph. */
int bpp_policy_heads_forward_train(const float *feat, int32_t n, const int32_t geom[], const float *weights, float *value, float *logits,
                                   float *pred, float *hidden, void *stream);

/* The backward of the above.
 *
 * feat, hidden, pred   what the forward read and wrote.
 * grad_value   f32 [n], grad_logits f32 [n][M], grad_pred f32 [n][M]: the gradients at the three outputs.  NULL: that head
 *              contributes nothing -- its slice of grad_feat, its rows of grad_hidden (and grad_out_mask for the mask head) and
 *              its weight gradients are written as zeros, not left alone.  At least one must be given.
 * weights_bwd  f32, bpp_policy_heads_backward_weights_floats(geom) floats: the six matrices packed for the input gradient, so
 *              that the 32 columns a wave loads for one k' are contiguous -- for these products torch's own [out][in] layout.
 *              No biases: the input gradient needs none.  Offsets in floats, W2 of a head directly in front of its W1:
 *
 *                dist.linear        [M][H]      at 0
 *                base.actor.3       [H][8 A]    at M H
 *                base.mask.5        [M][H]      at M H + 8 A H
 *                base.mask.3        [H][8 A]    at 2 M H + 8 A H
 *                base.critic_linear [1][H]      at 2 M H + 16 A H
 *                base.critic.3      [H][4 A]    at 2 M H + 16 A H + H
 *
 *              in all 2 M H + 20 A H + H floats.
 * grad_feat    f32 [n][20 A], written: the gradient at feat, exactly what bpp_policy_trunk_backward takes as grad_feat.  It is
 *              not masked by feat > 0: the trunk call applies that mask itself.
 * grad_hidden  f32 [3][n][H], written: the gradient at the pre-activation output of actor.3, mask.3, critic.3, laid out as hidden.
 * grad_out_mask f32 [n][M], written: the gradient at the pre-activation output of mask.5.
 *              With grad_logits and grad_value these are the G rows of all six layers as dense [R][D] arrays (BPP_KFAC_ROWS).
 * grad_weights f32 [bpp_policy_weights_floats(geom) - 151 380], written: the gradient of the forward blob from float 151 380 on in
 *              the blob's own layout -- every matrix [k][oc], the gradient of its bias behind it, in the order actor.3, dist.linear,
 *              mask.3, mask.5, critic.3, critic_linear.  Behind bpp_policy_trunk_backward's grad_weights it is the gradient of the
 *              whole blob.
 * workspace    bpp_policy_heads_backward_workspace(geom, n) bytes, 4-byte aligned; workspace_bytes: what the caller holds there.
 *              Holds nothing between calls.
 *
 * Normative arithmetic.  Everything is float32; nothing is fused except the fmaf chains.  W2 [Mh][H] and W1 [H][K1] are a head's
 * two matrices in torch's layout.
 *   go'_mask[b][m] = pred[b][m] > 0 ? grad_pred[b][m] : 0 (this is grad_out_mask); for the actor go' = grad_logits, for the critic
 *   go' = grad_value, one column.
 *   Dh[b][h] is ONE chain acc = fmaf(go'[b][m], W2[m][h], acc) over ascending m from +0.  Gh = hidden > 0 ? Dh : 0 (grad_hidden).
 *   grad_feat[b][f0 + k] is ONE chain over ascending h from +0 of fmaf(Gh[b][h], W1[h][k], acc).
 *   This is what v_mfma_f32_32x32x2_f32 computes, two k' per instruction.  A chain of odd length (M = A with S odd; the critic's
 *   single column) ends with one more step fmaf(0, w, acc) on the float behind the matrix, which the layout above keeps inside
 *   weights_bwd: it leaves the bits while that float is finite, as a tap outside the image does in bpp_policy_train.h.
 *   A row's grad_feat, grad_hidden and grad_out_mask depend on nothing but that row: the same bits alone and anywhere in a batch.
 *
 *   dW2[h][m] = sum over b of hidden[b][h] * go'[b][m];  dW1[k][h] = sum over b of feat[b][f0 + k] * Gh[b][h].  Each bias gradient
 *   is the row behind the matrix: the same product on an input value of 1, the chain fmaf(1, g, acc).
 *   Order: a split is `bins per split` = 128 consecutive bins, whatever geom and n are (the last split may be shorter).  Inside
 *   a split every element is ONE chain from +0 over ascending b.  A second kernel adds the partials of the splits in ascending
 *   split order in double and casts once to float.
 *   No atomic touches a sum: the same bits on every run, on another stream and in a replayed graph.
 *
 * Form.  The input-gradient kernel is the forward head kernel's sibling: a workgroup owns 64 bins and one head, go' passes
 * through LDS 64 features at a time, Gh stays in LDS between the two products.  The weight-gradient kernel gives a workgroup a
 * block of 64 rows k by 128 columns of one matrix [K + 1][OC] and one split; it stages 32 bins at a time, the input rows with
 * a column of ones behind feature K and the G rows, and reads the MFMA's A operand transposed from the former.
 *
 * BPP_E_BADARG, before any device is touched: a NULL pointer other than two of the three output gradients; what
 * bpp_policy_heads_forward_train refuses of n and geom; workspace_bytes smaller than bpp_policy_heads_backward_workspace(geom, n);
 * an n whose splits exceed the grid.
 * The call only enqueues three kernels on `stream`: no host wait, no allocation, capturable into a graph. */
int bpp_policy_heads_backward(const float *feat, const float *hidden, const float *pred, const float *grad_value, const float *grad_logits,
                              const float *grad_pred, int32_t n, const int32_t geom[], const float *weights_bwd, float *grad_feat,
                              float *grad_hidden, float *grad_out_mask, float *grad_weights, void *workspace, size_t workspace_bytes,
                              void *stream);

/* Bytes of `workspace`: splits * blocks * 8 tiles * 1024 floats (0 for arguments bpp_policy_heads_backward refuses). */
size_t bpp_policy_heads_backward_workspace(const int32_t geom[], int32_t n);

/* Floats of weights_bwd: 2 M H + 20 A H + H (0 for a geom that is refused). */
size_t bpp_policy_heads_backward_weights_floats(const int32_t geom[]);

/* The form bpp_policy_heads_backward takes (documentation and tests; touches no device; BPP_E_BADARG as above or for a NULL out):
 * out = {bins per workgroup of the input-gradient kernel (64), its LDS bytes, bins per split (128), splits, the longest chain of
 * the weight gradient in rows (min(n, bins per split)), LDS bytes of the weight-gradient kernel, path (1; 0 when refused, which a
 * non-NULL out is told as well), 64 x 128 blocks of all six matrices}. */
int bpp_policy_heads_backward_info(const int32_t geom[], int32_t n, int32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_POLICY_HEADS_TRAIN_H */
