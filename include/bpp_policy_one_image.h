/*
 * bpp_policy_one_image.h -- the CNNPro policy forward of bpp_policy.h on ONE LDS image per bin: the same
 * network, the same packed weights, the same workspace and the same normative arithmetic, for sides up to 22 (20 x 20 pallets).
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16) and to include/bpp_policy.h, whose symbols and refusals are
 * unchanged.  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_POLICY_ONE_IMAGE_H
#define BPP_POLICY_ONE_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Arguments, the packed blob, the workspace (n * 20 A floats), the optional heads and the normative arithmetic are exactly
 * those of bpp_policy_forward (include/bpp_policy.h): every output element of every layer is one float32 chain
 * acc = fmaf(x_k, w_k, acc) over ascending k, started from the bias.  Wherever both calls accept a shape they give the same bits.
 *
 * Form.  The trunk kernel gives a workgroup of four waves P bins (2 while the LDS stays within 80 KiB, which S <= 10 does; else
 * 1) and ONE image [64][(S + 2)^2 | 1] per bin with a zero halo, beside the two address tables of bpp_policy_forward.  A wave
 * owns TW = ceil(position tiles / 4) <= 4 tiles of 32 positions.  A layer is: every wave runs the whole k chain of all its tiles
 * and keeps the layer's output in the MFMA accumulators ([TW][2] tiles of 32 x 32); a barrier; every wave writes ReLU(acc) into
 * the interior of the image it read from; a barrier.  The 20 columns of the head convolutions go the same way: the features
 * [P][20 A] overwrite the start of the image behind the barrier and go to `workspace` in rows.  The head kernel is
 * bpp_policy_forward's.
 *
 *   S = 10, P = 2:   77 440 B of LDS (two workgroups share a compute unit), TW = 2
 *   S = 20, P = 1:  128 128 B (124 160 B of image), 13 tiles, TW = 4: 128 accumulator registers per lane
 *   S = 22, P = 1:  152 064 B, 16 tiles, TW = 4;  S = 23 would need 160 000 B of image alone
 *
 * BPP_E_BADARG, before any device is touched: a NULL obs / geom / weights / workspace; all three outputs NULL; n < 1; S < 1 or
 * S > 22; H < 1, H not a multiple of 32 or above 512; M not A or 2 A; obs_stride < 4 A.
 * The call only enqueues two kernels on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph. */
int bpp_policy_forward_one_image(const float *obs, int64_t obs_stride, int32_t n, const int32_t geom[], const float *weights, float *value,
                                 float *logits, float *pred, void *workspace, void *stream);

/* Bytes of `workspace`: n * 20 A floats (0 for arguments bpp_policy_forward_one_image refuses). */
size_t bpp_policy_forward_one_image_workspace(const int32_t geom[], int32_t n);

/* Floats of the packed blob, the layout of bpp_policy.h for this geom (0 for a geom bpp_policy_forward_one_image refuses). */
size_t bpp_policy_one_image_weights_floats(const int32_t geom[]);

/* The form bpp_policy_forward_one_image takes (documentation and tests; touches no device; BPP_E_BADARG as above or for a NULL
 * out): out = {bins per trunk workgroup P, trunk LDS bytes, trunk workgroups (ceil(n / P)), position tiles per wave TW, head
 * workgroups with all three heads (3 * ceil(n / 64)), side of an MFMA tile (32), position rows per trunk workgroup padded to
 * whole tiles, path (2; 0 when refused, which a non-NULL out is told as well)}. */
int bpp_policy_forward_one_image_info(const int32_t geom[], int32_t n, int32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_POLICY_ONE_IMAGE_H */
