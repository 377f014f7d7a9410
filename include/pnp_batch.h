/*
 * Batched entry points of the RANSAC-EPnP pose solver: part of the C ABI of include/pnp.h, which includes this file (include
 * pnp.h, not this file: the stream type and the conventions are declared there).
 */
#ifndef ONEPOSE_AMD_PNP_BATCH_H
#define ONEPOSE_AMD_PNP_BATCH_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a batch of frames in one chain of launches (pnp_version() >= 2) --------------------------------------------------
 * The kernels take the frame from the grid's y index and each frame's intrinsics, count and seed BY VALUE in the kernel
 * arguments, so one call enqueues four launches (five for the matches form) for all b frames.  The single-frame entry
 * points of pnp.h launch the same kernels with a batch of one.
 *
 * Shapes.   1 <= b <= PNP_MAX_ITEMS, cap >= 1, 0 <= n[i] <= cap.  Arrays are padded to the capacity: pts_3d [b][cap][3],
 *           pts_2d [b][cap][2], inlier_mask [b][cap], pose [b][12], info [b][4] on the device; K_host [b][9] doubles,
 *           n [b] and seeds [b] on the HOST (read during the call, free to reuse after it returns).
 * Padding.  Nothing past a frame's count is read; inlier_mask entries past the count are written as 0.
 * Short frames.  A frame with fewer than 5 correspondences (fewer than 5 valid matches) gets the identity pose,
 *           info = {0, 0, -1, 0} and a zero mask -- what pnp_ransac_epnp_matches answers for fewer than 5 valid matches.
 *           The call still returns 0 and the other frames are not affected.
 * Equality. Every frame's pose, inlier_mask and info are BITWISE those of pnp_ransac_epnp / pnp_ransac_epnp_matches called
 *           alone with that frame's K, seed and count: the same kernels run, no reduction's order depends on b, cap or
 *           another frame's count, and frame i's workspace slice starts at i * pnp_batch_workspace_bytes(1, cap, iterations).
 * Library.  Allocates nothing, copies nothing from the host beyond the by-value kernel arguments, never synchronises.
 * Errors.   Everything is validated before the first HIP call (so also on a machine without a GPU): -1 for a bad argument,
 *           -2 for a workspace shorter than pnp_batch_workspace_bytes(b, cap, iterations), each with pnp_last_error(). */
#define PNP_MAX_ITEMS 32
size_t pnp_batch_workspace_bytes(int b, int cap, int iterations); /* 0 for a shape it refuses */

int pnp_ransac_epnp_batch(const float* pts_3d, const float* pts_2d, const double* K_host, const int32_t* n,
                          const uint64_t* seeds, int b, int cap, double scale, double reproj_error, int iterations,
                          double* pose, int32_t* inlier_mask, int32_t* info, void* workspace, size_t workspace_bytes,
                          pnp_stream_t stream);

/* kpts2d [b][cap1][2], matches0 [b][cap1] (values in [-1, n3)), n1 [b] on the host: the query keypoints of each frame;
 * kpts3d [b][n3][3], or ONE database [n3][3] for all frames when shared3d == 1; inlier_mask [b][cap1] by query keypoint. */
int pnp_ransac_epnp_matches_batch(const float* kpts2d, const float* kpts3d, const int64_t* matches0, const double* K_host,
                                  const int32_t* n1, const uint64_t* seeds, int b, int cap1, int n3, int shared3d,
                                  double scale, double reproj_error, int iterations, double* pose, int32_t* inlier_mask,
                                  int32_t* info, void* workspace, size_t workspace_bytes, pnp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
