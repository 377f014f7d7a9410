/*
 * C ABI of the MI355X (gfx950) training head of the GATsSPG matcher, part of libgatsspg_hip.so (gtr_version() == 1).
 *
 * The matching head of one training step -- the score contraction, the dual softmax and the focal loss over the
 * b x n x m matrix, with its analytic backward -- i.e. the reference's
 *   src/models/GATsSPG_architectures/GATs_SuperGlue.py:217-218   scores = einsum(mdesc0, mdesc1) / scale; conf = softmax(1) * softmax(2)
 *   src/losses/focal_loss.py:13-26                               FocalLoss
 *   src/utils/data_utils.py:208-230                              reshape_assign_matrix (gtr_build_target)
 * under autograd.  x [b][256][n], y [b][256][m]: the L2-normalised matching descriptors, s = scale:
 *
 *   S_ij = <x_i, y_j> / s        E = exp(S)   (|S| <= 1/s: no maximum is subtracted; s < 1/80 is refused)
 *   r_i = sum_j E_ij   c_j = sum_i E_ij        A = E / c_j   B = E / r_i   C = A * B
 *   class 1 (positive):  l = -alpha (1-C)^gamma ln C         class 0 (negative):  l = -(1-alpha) C^gamma ln(1-C)
 *   class 2 (ignored):   in neither mean
 *   loss = pos_w * mean_pos(l) + neg_w * mean_neg(l)         means over the WHOLE batch; a term whose set is empty is dropped
 *   G = pos_w / N_pos * dl/dC on positives, neg_w / N_neg * dl/dC on negatives, 0 elsewhere;   H = G * C
 *   dS = 2 H - A * colsum_j(H) - B * rowsum_i(H)             dx = y dS^T / s      dy = x dS / s
 *
 * ONE DIFFERENCE from the reference: with no positive and no negative the reference asserts; here the loss is 0 and the
 * gradients are 0 (no host read-back).  ln(1 - C) is logf(1 - C) in fp32 as the reference's; gamma == 2 is a product,
 * any other gamma goes through exp2 / log2.
 *
 * Launch chain of gtr_loss_head: pack (x, y into zero-padded planes; y also transposed) | score tile kernel on the fp32
 * MFMA main loop, 128 x 64 tiles: E = exp, written once to the workspace, with row / column sum partials per tile |
 * r, c | one streaming pass over E and the classes: loss sums, counts, rowsum / colsum partials of H | loss and counts
 * (fp64 combine) | rowsum(H), colsum(H) | one streaming pass that overwrites E with dS | two GEMM launches on the
 * same main loop (dx contracts over m, dy over n; K zero-padded to whole slabs).  Without dx and dy the chain stops
 * after the loss.  Every sum runs in a fixed order that depends on the shape alone; there are no floating-point
 * atomics: two calls are bitwise equal.  fp32 arithmetic (v_mfma_f32_32x32x2_f32 + fp32 VALU) only.
 *
 * Conventions as in gatsspg.h: device pointers unless marked host, a caller workspace of gtr_workspace_bytes (256-byte
 * aligned) that may hold anything on entry, work enqueued on `stream`, no allocation, no synchronisation, 0 = OK /
 * negative = error (-1 bad argument, -2 workspace too small, -3 launch failed) + gtr_last_error().
 *
 * Limits: 1 <= b <= GTR_MAX_BATCH, 1 <= n, m <= GTR_MAX_POINTS, n * m <= GTR_MAX_ELEMENTS.
 */
#ifndef ONEPOSE_AMD_GATSSPG_TRAIN_H
#define ONEPOSE_AMD_GATSSPG_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTR_DESC_DIM 256
#define GTR_MAX_BATCH 64
#define GTR_MAX_POINTS 4194304    /* 2^22 per side: the tile kernels address a 128-row panel with 32-bit byte offsets */
#define GTR_MAX_ELEMENTS 67108864 /* 2^26 = n * m */
#define GTR_CLASS_NEGATIVE 0
#define GTR_CLASS_POSITIVE 1
#define GTR_CLASS_IGNORED 2

int gtr_version(void);
const char* gtr_last_error(void);

/* Bytes of workspace every entry point below takes for (b, n, m); 0 = refused (gtr_last_error() says why). */
size_t gtr_workspace_bytes(int b, int n, int m);

/* reshape_assign_matrix on the device.  pairs [b][2][kcap] int32 (device): row 0 the 2D index, row 1 the 3D index; k,
 * n_orig, m_orig [b] (HOST): the pairs of sample i are its first k[i] columns, its unpadded shape is n_orig[i] x m_orig[i].
 * cls [b][n][m] <- 1 where a pair names the entry, 0 elsewhere, then rows >= n_orig and columns >= m_orig <- the pad
 * class (pad_is_negative ? 0 : 2), also where a positive was set (data_utils.py:220-221).  A pair with an index >= the
 * shape is dropped (:216), duplicates are one entry.  ONE DIFFERENCE: a negative index (which torch wraps around) is
 * ignored; negative_pairs [1] (may be NULL) <- how many pairs had one.  Plain stores, no atomics. */
int gtr_build_target(const int32_t* pairs, const int32_t* k, const int32_t* n_orig, const int32_t* m_orig, int b, int kcap, int n, int m,
                     int pad_is_negative, int8_t* cls, int32_t* negative_pairs, void* stream);

/* The whole head.  cls [b][n][m] int8 (GTR_CLASS_*; any other value counts as ignored).  alpha in [0, 1], gamma > 0,
 * pos_w, neg_w >= 0, scale >= 1/80, all finite.  loss [1], counts [3] int64 (positives, negatives, ignored); dx
 * [b][256][n] and dy [b][256][m] are written when BOTH are non-NULL (both NULL: forward only). */
int gtr_loss_head(const float* x, const float* y, const int8_t* cls, int b, int n, int m, double alpha, double gamma, double pos_w,
                  double neg_w, double scale, float* loss, int64_t* counts, float* dx, float* dy, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Stage: E [b][n][m] = exp(<x_i, y_j> / scale), r [b][n], c [b][m] (pack, score tile kernel, finalise). */
int gtr_scores_exp(const float* x, const float* y, int b, int n, int m, double scale, float* E, float* r, float* c, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Stage: from E, r, c and the classes: loss_sums [2] fp64 (sum of l over the positives, over the negatives), counts [3],
 * loss [1] (the combined loss), rowsum_h [b][n] = rowsum_i(H), colsum_h [b][m] = colsum_j(H). */
int gtr_loss_terms(const float* E, const float* r, const float* c, const int8_t* cls, int b, int n, int m, double alpha, double gamma,
                   double pos_w, double neg_w, double* loss_sums, int64_t* counts, float* loss, float* rowsum_h, float* colsum_h,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Stage: dS [b][n][m] from E, r, c, the classes, the counts [3] and the H sums of gtr_loss_terms. */
int gtr_score_grad(const float* E, const float* r, const float* c, const int8_t* cls, const int64_t* counts, const float* rowsum_h,
                   const float* colsum_h, int b, int n, int m, double alpha, double gamma, double pos_w, double neg_w, float* dS,
                   void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
