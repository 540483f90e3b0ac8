/*
 * bpp_policy.h -- the CNNPro policy forward for inference as two kernels: the network of acktr/model.py:265-323
 * (five 3x3 convolutions 4 -> 64 -> 64 -> 64 -> 64 -> 64 with ReLU, three 1x1 head convolutions with ReLU, two Linear layers per
 * head) and dist.linear (acktr/distributions.py:72), float32 on the matrix cores.  The trunk runs inside the LDS of one workgroup
 * and no trunk activation ever reaches memory; only the 20 * A head features of a bin do.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_POLICY_H
#define BPP_POLICY_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* geom = {S, H, M}: S the pallet side (the image is S x S, A = S * S positions), H the hidden size, M = A or 2 A the number of
 * actions (= the length of the mask prediction).  The input has 4 channels and the trunk is 64 wide.
 *
 * obs      f32, row b at obs + b * obs_stride (floats, >= 4 A): the environment's observation row, read as [4][S][S] (model.py:316).
 * weights  f32, ONE packed blob of bpp_policy_weights_floats(geom) floats on the device.  Every weight matrix is stored [k][oc]
 *          (the transpose of torch's weight.view(OC, -1): k = c * 9 + i * 3 + j for a 3x3 convolution, k = c for a 1x1, k = the
 *          input feature of a Linear), so the 32 columns a wave loads for one k are contiguous; the bias [oc] follows its matrix.
 *          Layers in this order, offsets in floats:
 *
 *            share.0       W [36][64]   b [64]        at 0
 *            share.2       W [576][64]  b [64]        at 2368
 *            share.4       W [576][64]  b [64]        at 2368 + 36928
 *            share.6       W [576][64]  b [64]        at 2368 + 2 * 36928
 *            share.8       W [576][64]  b [64]        at 2368 + 3 * 36928
 *            head convs    W [64][20]   b [20]        at 150080: columns 0-7 actor.0, 8-15 mask.0, 16-19 critic.0
 *            actor.3       W [8 A][H]   b [H]         at 151380
 *            dist.linear   W [H][M]     b [M]         then each directly after the one before
 *            mask.3        W [8 A][H]   b [H]
 *            mask.5        W [H][M]     b [M]
 *            critic.3      W [4 A][H]   b [H]
 *            critic_linear W [H][1]     b [1]
 *
 *          The input feature of actor.3 / mask.3 / critic.3 is c * A + y * S + x, the order of Flatten over [C][S][S].
 * value    f32 [n]     critic_linear(critic(share))
 * logits   f32 [n][M]  dist.linear(actor(share)), before any masking
 * pred     f32 [n][M]  mask(share), including its final ReLU
 *          Each may be NULL (at least one is not): a head whose pointer is NULL is not computed.
 *
 * Normative arithmetic.  Every output element of every layer is ONE float32 chain acc = fmaf(x_k, w_k, acc) over ascending k in
 * the order above, started from acc = bias; a tap outside the image contributes fmaf(0, w, acc); ReLU is acc > 0 ? acc : 0.
 * This is what v_mfma_f32_32x32x2_f32 computes, two k per instruction.  There is no split of k, no atomic, and no dependence on
 * n, on the bin's place in the batch or on the other bins of its workgroup: the same bits on every run and in a replayed graph,
 * and a bin's outputs are the same bits whatever batch it is evaluated in.
 *
 * Form.  The trunk kernel gives a workgroup P bins (bpp_policy_forward_info; 2 at S = 10): two images [64][(S + 2)^2 | 1] per
 * bin with a zero halo live in LDS and the five layers go back and forth between them; the A operand of the MFMA is read from
 * the image at `offset of the feature + offset of the position`, the B operand from the blob.  The head features
 * [20 A] = actor [8][A], mask [8][A], critic [4][A] of each bin go to `workspace`.  The head kernel gives a workgroup 64 bins and
 * one head: features -> hidden (kept in LDS) -> output.
 *
 * workspace: bpp_policy_forward_workspace(geom, n) bytes (n * 20 A floats), 4-byte aligned; holds nothing between calls.
 *
 * BPP_E_BADARG, before any device is touched: a NULL obs / geom / weights / workspace; all three outputs NULL; n < 1; S < 1 or
 * H < 1; M not A or 2 A; obs_stride < 4 A; H not a multiple of 32 or above 512; a side whose two images for one bin do not fit
 * the 160 KiB of LDS (S > 15: 20 x 20 is refused).
 * The call only enqueues two kernels on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph. */
int bpp_policy_forward(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *value,
                       float *logits, float *pred, void *workspace, void *stream);

/* Bytes of `workspace` (0 for arguments bpp_policy_forward refuses). */
size_t bpp_policy_forward_workspace(const int32_t geom[], int32_t n);

/* Floats of the packed blob (0 for a geom bpp_policy_forward refuses). */
size_t bpp_policy_weights_floats(const int32_t geom[]);

/* The form bpp_policy_forward takes (documentation and tests; touches no device; BPP_E_BADARG as above or for a NULL out):
 * out = {bins per trunk workgroup P, trunk LDS bytes, trunk workgroups, bins per head tile T (64), head workgroups with all
 * three heads (3 * ceil(n / T)), side of an MFMA tile (32), position rows per trunk workgroup padded to whole tiles, path
 * (1; 0 when refused, which a non-NULL out is told as well)}. */
int bpp_policy_forward_info(const int32_t geom[], int32_t n, int32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_POLICY_H */
