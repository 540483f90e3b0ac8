/*
 * bpp_kfac.h -- one Kronecker factor of K-FAC and its running average as two kernels: the covariance
 * X^T X of the rows the reference's compute_cov_a / compute_cov_g build (acktr/algo/kfac.py:28-63, fast_cnn=False), folded into
 * the running statistic by update_running_stat (kfac.py:66-70).  The rows of a Conv2d input factor are im2col patches
 * (kfac.py:15-25); they are formed in LDS from the staged image by address arithmetic and never written anywhere.
 *
 * Additive to include/bpp_abi.h (BPP_ABI_VERSION stays 16).  Only libbpp_hip.so exports these symbols.
 */
#ifndef BPP_KFAC_H
#define BPP_KFAC_H

#include <stddef.h>
#include <stdint.h>

#include "bpp_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Source layouts.  A row is one summand of the covariance, D the side of the factor, R the number of rows.
 *
 *   BPP_KFAC_PATCH  src f32 [B][C][H][W], geom = {B, C, H, W, kh, kw, sh, sw, ph, pw}.  Row (b, oy, ox) is the im2col patch of
 *                   output position (oy, ox) of sample b: feature c * kh * kw + i * kw + j = src[b][c][oy * sh - ph + i][ox * sw - pw + j],
 *                   0 outside the image -- the order of _extract_patches and of weight.view(OC, -1).
 *                   OH = (H + 2 ph - kh) / sh + 1, OW alike; D = C * kh * kw, R = B * OH * OW.
 *   BPP_KFAC_ROWS   src f32 [R][D] dense, geom = {R, D}: the inputs or grad-outputs of a Linear, or bias gradients summed
 *                   over space.
 *   BPP_KFAC_NCHW   src f32 [B][D][S], geom = {B, D, S}.  Row (b, s), feature d = src[b][d][s]: what
 *                   g.transpose(1, 2).transpose(2, 3).view(-1, OC) gives for a conv grad-output with S = OH * OW.  R = B * S. */
#define BPP_KFAC_PATCH 0
#define BPP_KFAC_ROWS 1
#define BPP_KFAC_NCHW 2

/* m [D][D] f32, in and out:
 *
 *   aa[i][j] = scale * sum_r x[r][i] * x[r][j]
 *   first != 0:  m = aa                                        (kfac.py:159-162, :177-180)
 *   m = ((m * c1) + aa) * c2, c1 = (float)(stat_decay / (1 - stat_decay)), c2 = (float)(1 - stat_decay), float32, unfused
 *                                                              (update_running_stat, kfac.py:66-70)
 *
 * `scale` is the product of the reference's scalings, formed in double by the caller:
 *   Conv2d input (PATCH):        1 / (B * (OH * OW)^2)   rows / OH / OW (kfac.py:38), then a^T @ (a / B) (:45)
 *   Conv2d grad-output (NCHW):   B * OH * OW             rows * OH * OW (:57), * B (:62), / rows with rows = B * OH * OW (:63)
 *   Linear grad-output (ROWS):   B                       * B (:62), / B (:63); the same for a summed bias gradient (:59-63)
 *   Linear input (ROWS):         1 / B                   (:45)
 *
 * Normative order of the sum.  Rows are taken in units: a sample for PATCH; for NCHW one of the ceil(S / 64) chunks of
 * ceil(S / chunks) consecutive positions a sample is cut into (the last chunk takes what is left); 64 consecutive rows for
 * ROWS.  A split is a fixed number of consecutive units, the same for every split but the last, out[3] rows; the numbers
 * depend on layout and geom alone (bpp_kfac_factor_info).  Inside a split an output element is ONE
 * float32 chain over its rows in ascending order, acc = fmaf(x[r][i], x[r][j], acc) from acc = +0: what
 * v_mfma_f32_32x32x2_f32 computes, two rows per instruction.  (A unit with an odd number of rows ends with one
 * fmaf(0, 0, acc).)  A second kernel adds the partial sums of the splits in ascending split order in double, multiplies by
 * `scale` in double and casts once to float; then the update above.  No atomic touches a sum: the same bits on every run.
 *
 * Only output tiles with column tile >= row tile are computed, and inside a diagonal tile only elements with j >= i are
 * used: m[i][j] and m[j][i] are written from the one value and are the same bits.  Of the incoming m only the upper triangle
 * (j >= i) is read.
 *
 * workspace: bpp_kfac_factor_workspace(layout, geom) bytes, 8-byte aligned; holds nothing between calls.
 *
 * BPP_E_BADARG, before any device is touched: a NULL src / geom / m / workspace, an unknown layout, D < 1 or R < 1 (any
 * extent < 1), stride < 1, padding < 0, a kernel larger than the padded image, R or the element count of src beyond
 * 2^31 - 1 rows / 2^62 elements, stat_decay outside (0, 1), a PATCH image whose staged channels do not fit 64 KiB of LDS.
 * The call only enqueues two kernels on `stream` (a hipStream_t): no host wait, no allocation, capturable into a graph. */
int bpp_kfac_factor(const float *src, int32_t layout, const int32_t geom[], float *m, double scale, double stat_decay, int32_t first,
                    void *workspace, void *stream);

/* Bytes of `workspace` (0 for arguments bpp_kfac_factor refuses). */
size_t bpp_kfac_factor_workspace(int32_t layout, const int32_t geom[]);

/* The form bpp_kfac_factor takes (documentation and tests; touches no device; BPP_E_BADARG as above or for a NULL out):
 * out = {D, R, side of an output tile (32), rows per split, splits, chain length = the most rows one chain of fmaf runs
 * over = min(rows per split, R)}. */
int bpp_kfac_factor_info(int32_t layout, const int32_t geom[], int32_t out[6]);

#ifdef __cplusplus
}
#endif

#endif /* BPP_KFAC_H */
