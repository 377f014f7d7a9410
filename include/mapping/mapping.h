/*
 * C ABI of the MI355X (gfx950) object database builder -- the tail of OnePose's SfM preprocessing
 * (run.py:80-163) behind SuperPoint and SuperGlue: geometric verification of the 2D-2D matches with
 * the known poses, triangulation of the feature tracks with every camera fixed, the track-length /
 * 3D-box / 1 mm merge filters (src/sfm/postprocess/filter_tkl.py, filter_points.py) and the descriptor
 * collection and averaging (feature_process.py:95-188, 297-317).
 *
 * The reference hands verification and triangulation to COLMAP (matches_importer, point_triangulator:
 * src/sfm/triangulation.py:117-135,179-180), an external binary that is neither vendored by the
 * reference nor installed here.  The kernels restate the published form of what it is asked to do:
 *   - verification: a match survives when each keypoint lies within max_epipolar_error pixels of the
 *     epipolar line of the other, the epipolar geometry taken from the KNOWN poses;
 *   - triangulation: RANSAC over two-view midpoints (every pair of a short track, hash-sampled pairs
 *     of a long one), inliers by positive depth and squared reprojection error, most inliers wins,
 *     lowest hypothesis index on ties; refit = linear multi-ray least squares, then Gauss-Newton steps
 *     on the reprojection error over the inliers.  With every camera and intrinsic held fixed, as the
 *     reference asks of COLMAP (triangulation.py:127-129), bundle adjustment decouples into exactly
 *     this per-point problem.
 * NOT claimed: parity with COLMAP itself.  Known differences: verification uses the known poses, not
 * a RANSAC-estimated two-view geometry; tracks (built by the caller) are whole connected components;
 * the minimal solver is the midpoint, not the DLT; the residual is the reprojection error throughout;
 * all candidate pairs are scored, not a confidence-bounded subset; there is no re-triangulation /
 * track-merging pass.  Nobody has measured the difference: the binary is not here.
 *
 * All geometry is fp64 on fp32 keypoints, compiled without FMA contraction: tests/mapping_oracle.py
 * restates every expression in the same order in numpy.
 *
 * Cameras: `cams` [V][16] double (device): the world->camera pose [R | t] row-major 3x4 (12 numbers),
 * then fx, fy, cx, cy of a pinhole K.
 *
 * Conventions as in pnp.h and detector.h: device pointers, caller-provided workspace, work enqueued
 * on `stream`, no allocation, no synchronisation, 0 = OK / non-zero = error + map_last_error().
 */
#ifndef ONEPOSE_AMD_MAPPING_H
#define ONEPOSE_AMD_MAPPING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* map_stream_t; /* hipStream_t */

#define MAP_MAX_TRACK_LENGTH 448 /* observations of one track (staged in LDS) */
#define MAP_MAX_POINTS 32768     /* points map_merge_points accepts */
#define MAP_MAX_LENGTH_BINS 1024 /* track lengths >= this share the last histogram bin */

int map_version(void);
const char* map_last_error(void);

/* bytes of workspace map_merge_points needs for n points (the n x n adjacency bits); 0 = refused.
 * No other entry point needs a workspace. */
size_t map_workspace_bytes(int n_points);

/* Geometric verification of P image pairs in one launch (one workgroup per pair).
 *   kpts [sum n_v][2] fp32: the keypoints of all images, image after image; kpt_offsets [V+1] int32;
 *   pair_images [P][2] int32: (i, j); match_offsets [P+1] int32: pair p owns matches0[match_offsets[p] ..
 *   match_offsets[p+1]), one entry per keypoint of image i (at most n_i are read): index into image j or -1
 *   (entries >= n_j count as unmatched).
 *   A match (a, b) survives when the squared distance of kpts_j[b] to the epipolar line of kpts_i[a] and that of
 *   kpts_i[a] to the line of kpts_j[b] are both <= max_epipolar_error^2.
 *   out_matches [match_offsets[P]][2] int32: the survivors of pair p as (a, b), compacted in index order from row
 *   match_offsets[p]; counts [P] int32: survivors, 0 when fewer than min_pair_inliers survive (rows then undefined). */
int map_verify_matches(const float* kpts, const int32_t* kpt_offsets, const double* cams, int V, const int32_t* pair_images,
                       const int32_t* match_offsets, const int64_t* matches0, int P, double max_epipolar_error,
                       int min_pair_inliers, int32_t* out_matches, int32_t* counts, map_stream_t stream);

/* Triangulation of T tracks in CSR form.
 *   track_offsets [T+1] int32; obs_image [M] int32; obs_xy [M][2] fp32; max_track_length: an upper bound of the track
 *   lengths known to the caller, <= MAP_MAX_TRACK_LENGTH: it sizes the LDS of the long tracks.  A track longer than it,
 *   rounded up to a multiple of 64, is reported ok = 0 and never read past; so is one with fewer than 2 observations or
 *   with an image index outside [0, V).
 *   Hypotheses of a track of m observations: every pair (a < b) in lexicographic order when m (m - 1) / 2 <=
 *   max_hypotheses, otherwise max_hypotheses pairs drawn with the hash of ransac_sample.h (duplicates rejected).
 *   xyz [T][3] double (zeros when ok = 0); inlier_mask [M] int32: the observations kept after the refit;
 *   info [T][4] int32: {ok, m, index of the best hypothesis (-1 when none is valid), its inlier count};
 *   lengths [T] int32: observations kept (0 when ok = 0) -- the track length the filters below use.
 * Tracks of up to 64 observations run on one wave each, longer ones on one workgroup each (both launches span all T tracks
 * and a workgroup returns at once for a track of the other class; the second is skipped when max_track_length <= 64);
 * the threshold and filter stages are one workgroup walking all T, sized for tens of thousands of tracks; sums are fixed-order trees:
 * a track's result does not depend on the batch it is launched in. */
int map_triangulate_tracks(const int32_t* track_offsets, const int32_t* obs_image, const float* obs_xy, const double* cams, int T,
                           int V, int max_track_length, double max_reproj_error, double min_tri_angle_deg, int max_hypotheses,
                           int refine_iterations, uint64_t seed, double* xyz, int32_t* inlier_mask, int32_t* info,
                           int32_t* lengths, map_stream_t stream);

/* filter_tkl.py:42-50 as written: lengths [T] int32 (0 = no point); remaining = number of points; walking the occurring
 * lengths in ascending order and subtracting each one's count, the first length at which remaining <= max_num_kp3d.
 * threshold [1] int32 (device); 0 when there is no point. */
int map_track_length_threshold(const int32_t* lengths, int T, int max_num_kp3d, int32_t* threshold, map_stream_t stream);

/* filter_points.py:8-72: keep point i when lengths[i] > 0, lengths[i] >= *threshold and it lies strictly inside the box:
 * fp32 test on the point cast to fp32, p' = p - c4, edges v45, v40, v47 from corner 4, 0 < p'.v < v.v.
 *   xyz [T][3] double; threshold [1] int32 (device); box_corners_host: 24 floats on the HOST, [8][3];
 *   kept_ids [T] int32 ascending, kept_xyz [T][3] fp32 (the fp32-rounded coordinates), count [1] int32 (device). */
int map_filter_points(const double* xyz, const int32_t* lengths, int T, const int32_t* threshold, const float* box_corners_host,
                      int32_t* kept_ids, float* kept_xyz, int32_t* count, map_stream_t stream);

/* filter_points.py:86-117: adjacency bits ||p_i - p_j|| < dist_threshold (fp64 sqrt((dx^2 + dy^2) + dz^2) on the fp32
 * coordinates), then the greedy sweep in index order: row j founds a new point unless a member of its row is already
 * taken; the new point is the fp32 mean of the row summed in index order.
 *   xyz32 [n][3] fp32; merged_xyz [n][3] fp32; member_offsets [n+1] int32 (entries past the merged count undefined);
 *   members [n] int32: positions 0..n-1 in ascending order per merged point; count [1] int32 (device): merged points. */
int map_merge_points(const float* xyz32, int n, double dist_threshold, float* merged_xyz, int32_t* member_offsets,
                     int32_t* members, int32_t* count, void* workspace, size_t workspace_bytes, map_stream_t stream);

/* feature_process.py:95-188, 297-317: collected and averaged descriptors.
 *   desc_table [V] pointers (device array of device pointers) to [dim][n_v] fp32; score_table [V] pointers to [n_v]
 *   fp32; n_kpts [V] int32; point_offsets [N+1] int32; obs_image / obs_kpt [K] int32: the observations of point i in the
 *   reference's traversal order (merged member after member, image order inside).
 *   collect_desc [K][dim] fp32, collect_scores [K] fp32, idxs [N] int64, mean_desc [N][dim] double, mean_scores [N]
 *   double: sums in that order in fp64, divided by the count.  An observation out of range gives zeros. */
int map_gather_descriptors(const float* const* desc_table, const float* const* score_table, const int32_t* n_kpts, int V,
                           const int32_t* point_offsets, const int32_t* obs_image, const int32_t* obs_kpt, int N, int dim,
                           float* collect_desc, float* collect_scores, int64_t* idxs, double* mean_desc, double* mean_scores,
                           map_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
