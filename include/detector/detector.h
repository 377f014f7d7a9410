/*
 * C ABI of the MI355X (gfx950) 2D object detector tail -- what OnePose's LocalFeatureObjectDetector
 * (src/local_feature_2D_detector/local_feature_2D_detector.py) does after its SuperGlue forwards:
 * match selection, cv2.estimateAffinePartial2D, the box vote, the two cv2.warpAffine crops and
 * get_K_crop_resize.  Everything stays in HBM between the matcher and the crop.
 *
 * The algorithms live in OpenCV (not vendored by the reference, not installed here).  The kernels
 * restate their published form in fp64, like the reference's float64 cv2 results:
 *   - partial affine  x' = [[a, -b], [b, a]] x + t  (4 DoF) inside OpenCV's RANSAC scheme: minimal
 *     sets of 2 matches, inlier when the squared reprojection error is <= threshold^2, most inliers
 *     wins, lowest hypothesis index on ties, one refit over the inliers.
 *   Three documented differences from cv2.estimateAffinePartial2D:
 *     1. sample indices come from a counter-based hash (splitmix64 over seed, hypothesis and draw
 *        counter, duplicates rejected): cv::RNG cannot be reproduced without OpenCV;
 *     2. every one of the `iterations` hypotheses is evaluated (OpenCV stops at its adaptive
 *        confidence bound: a subset of this search);
 *     3. OpenCV refines with 10 Levenberg-Marquardt steps; the squared error of this model is
 *        linear in (a, b, tx, ty), so the refit is the closed-form least squares over the inliers
 *        (the fixed point LM converges to).
 *     Samples whose two source points coincide are skipped.
 *   - the crop: both warps of crop_img_by_bbox folded into one exact-integer bilinear resampling
 *     (see det_crop_resize).
 * NOT claimed: parity with OpenCV itself.  cv2.warpAffine quantises sampling positions to 1/32 px
 * and weights to 15 bits, cv2.getAffineTransform solves a 6x6 system numerically, and
 * estimateAffinePartial2D differs as listed above.  Nobody has measured those differences here (no
 * cv2 on the development machines); tests/test_det_cv2.py records them where cv2 exists.
 *
 * Conventions as in pnp.h: device pointers, caller-provided workspace, work enqueued on `stream`,
 * no allocation, no synchronisation, 0 = OK / non-zero = error + det_last_error().
 */
#ifndef ONEPOSE_AMD_DETECTOR_H
#define ONEPOSE_AMD_DETECTOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* det_stream_t; /* hipStream_t */

#define DET_RANK_BY_MATCHES 0 /* the reference as written: local_feature_2D_detector.py:139-147 */
#define DET_RANK_BY_INLIERS 1 /* deviation: rank views by RANSAC inliers */
#define DET_MIN_MATCHES 6     /* local_feature_2D_detector.py:93 */

int det_version(void);
const char* det_last_error(void);

/* bytes of workspace for V views of at most cap0 matches each (iterations only range-checked); 0 = refused */
size_t det_workspace_bytes(int V, int cap0, int iterations);

/* cv2.estimateAffinePartial2D(src, dst, ransacReprojThreshold = reproj_threshold)  (local_feature_2D_detector.py:104-106)
 * on point lists; stage tests.
 *   src, dst [n][2] fp32 (device); affine [6] double (device): row-major 2x3 [[a, -b, tx], [b, a, ty]], zeros when ok = 0;
 *   inlier_mask [n] int32 (device): 1 for the inliers of the best hypothesis (before the refit, like cv2's mask);
 *   info [4] int32 (device): {ok, n, index of the best hypothesis (-1 when ok = 0), its inlier count}.
 *   ok = 0 when n < 2 or no sample with two distinct source points exists.
 * det_workspace_bytes(1, n, iterations) sizes the workspace. */
int det_affine_partial_ransac(const float* src, const float* dst, int n, double reproj_threshold, int iterations, uint64_t seed,
                              double* affine, int32_t* inlier_mask, int32_t* info, void* workspace, size_t workspace_bytes,
                              det_stream_t stream);

/* The same fit for V reference views in one launch, straight from the matcher's outputs, with the selection of
 * local_feature_2D_detector.py:85-90 done on the device in index order
 * (valid = matches0 > -1; mkpts0 = kpts0[valid]; mkpts1 = kpts1[matches0[valid]]):
 *   kpts0    [V][cap0][2] fp32: keypoints of the reference views, padded; n0 [V] int32 (device): keypoints of view v;
 *   matches0 [V][cap0] int64: index into kpts1 or -1 (entries >= n1 count as unmatched);
 *   kpts1    [n1][2] fp32: keypoints of the query frame, shared by all views;
 *   affine [V][6], inlier_mask [V][cap0] (indexed by REFERENCE-VIEW keypoint), info [V][4] = {ok, n_matches, best index,
 *   n_inliers} as above; ok = 0 when n_matches < DET_MIN_MATCHES (:93) or no non-degenerate sample exists (the reference
 *   would raise on `None @ ...`; treated like the < 6 branch). */
int det_affine_partial_from_matches(const float* kpts0, const int32_t* n0, const int64_t* matches0, const float* kpts1, int V,
                                    int cap0, int n1, double reproj_threshold, int iterations, uint64_t seed, double* affine,
                                    int32_t* inlier_mask, int32_t* info, void* workspace, size_t workspace_bytes,
                                    det_stream_t stream);

/* Box per view and the vote (local_feature_2D_detector.py:108-147):
 *   hw0 [V][2] int32 (device): (H0, W0) of each reference view; its corners (0,0) (W0,0) (0,H0) (W0,H0) go through the
 *   refit affine, are truncated toward zero like .astype(np.int32) (:117; clamped to the int32 range), min / max ->
 *   [x0, y0, x1, y1].  Views with ok = 0 give [0, 0, query_h, query_w], exactly as :98 has it (x1 = H, y1 = W).
 *   The vote keeps the view with the largest key, the first view among equals (Python's stable sorted(reverse=True)):
 *   DET_RANK_BY_MATCHES: key = n_matches (0 for ok = 0) -- the reference ranks by inliers.shape[0] of cv2's N x 1 mask,
 *   i.e. by the number of MATCHES; DET_RANK_BY_INLIERS: key = n_inliers (a deviation).
 *   boxes [V][4] int32, bbox [4] int32, best_view [1] int32: device. */
int det_bbox_vote(const double* affine, const int32_t* info, const int32_t* hw0, int V, int query_h, int query_w, int rank_by,
                  int32_t* boxes, int32_t* bbox, int32_t* best_view, det_stream_t stream);

/* crop_img_by_bbox + get_K_crop_resize (local_feature_2D_detector.py:160-186, data_utils.py:24-57,233-272) in one kernel.
 * With rot = 0 get_affine_transform scales both axes by dst_w / src_w and maps centre to centre, so for w = x1 - x0,
 * h = y1 - y0:  stage 1 is the integer translation (-x0, -y0) (an exact crop, zero outside the image) and stage 2 is
 * s = crop / w on both axes with ty = crop / 2 - s h / 2.  Output pixel (u, v) samples the w x h crop bilinearly at
 * (u w / crop, (v - crop / 2) w / crop + h / 2), value 0 outside the crop rectangle and outside the image
 * (BORDER_CONSTANT).  crop_size must be a power of two in [2, 2048]: positions and weights are then exact multiples of
 * 1 / crop, the weighted sum of uint8 samples is an int32, rounded half to even to a grey level, written as level / 255.
 *   image_u8 [H][W] uint8 (device); bbox [4] int32 (device); K_host: 9 doubles on the HOST, row-major;
 *   out [crop][crop] fp32 (device); K_crop [9] double (device) = M2 M1 K;
 *   info [4] int32 (device): {ok, w, h, 0}; ok = 0 (zero image, zero K_crop) when w <= 0 or h <= 0. */
int det_crop_resize(const uint8_t* image_u8, int H, int W, const int32_t* bbox, const double* K_host, int crop_size, float* out,
                    double* K_crop, int32_t* info, det_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
