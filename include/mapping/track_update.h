/*
 * C ABI of the MI355X (gfx950) map update step of the keyframe tracker, part of libmap_hip.so (map_version() >= 3).
 *
 * Replaces, on the GPU, the block of the reference's BATracker.track_ba that turns one frame's 2D-2D matches into the
 * next bundle-adjustment problem,
 *   src/tracker/ba_tracker.py:499-603  (and :251-273 _triangulatePy / apply_triangulation, :686 the unmatched list),
 * with `project` of src/tracker/tracking_utils.py:74-88.  The algorithm below is stated as OURS; every rule names the
 * reference line it follows.  The pair order is ascending keyframe index throughout.
 *
 *   1. Pairs (:499-503).  Pair k is the k-th i with 0 <= matches0[i] < n_q, its j = matches0[i].  A value >= n_q or
 *      < -1 is counted as ignored and makes no pair.  m = the number of pairs.
 *   2. Class (:518-526).  id = kf_pt_ids[i]: 0 <= id < n_points: KNOWN; id == -1: CANDIDATE; anything else is counted
 *      as ignored and the pair gets id -1.
 *   3. Known pairs (:530-543).  d = |project(points[id], K_q, pose_q) - q_xy[j]|.  project: Xc_r = (R_r0 X_0 + R_r1 X_1)
 *      + R_r2 X_2, then + t_r; h_r = (K_r0 Xc_0 + K_r1 Xc_1) + K_r2 Xc_2 with the full 3x3 K; x = h_0 / h_2, y = h_1 / h_2.
 *      d = sqrt(dx dx + dy dy).  med = gate_factor x median(d), numpy's median: the middle order statistic for an odd
 *      count, (a + b) / 2 of the two middle ones for an even count, NaN when any d is NaN or there is no known pair.
 *      The pair keeps its id iff d < med.  Selection: a radix select on the order-preserving integer key of the doubles,
 *      two bits a pass from the top, integer counts only.
 *   4. Candidates (:548-583, :251-265).  P = K pose[:3] for both views (row dots, index ascending); the rows of A as at
 *      :255-259 (view 1 = keyframe, view 2 = query); M = A^T A summed over the rows in ascending order; the eigenvector
 *      of the smallest eigenvalue (ties: lowest index) by cyclic Jacobi on the packed 4x4 (stops when the off-diagonal
 *      mass is not above 1e-30 of the diagonal mass, at most 16 sweeps); X = v[:3] / v[3]; rep_q, rep_kf by project into
 *      both views.  Removed when rep_q > max_reproj, rep_kf > max_reproj or X[2] > max_z.
 *      ONE DIFFERENCE from the reference: also removed when any of X, rep_q, rep_kf is not finite (the reference's `>`
 *      tests let NaN through into the bundle adjustment, which then refuses the whole start).  Counted in summary[5].
 *   5. Ids (:586-598).  The r-th kept candidate in pair order gets id n_points + r, its X goes to new_points[r].
 *   6. Unmatched (:686).  The ascending list of query indices no pair names.  Two pairs may name one j; both stand.
 *
 * NOT claimed: parity with cv2.triangulatePoints (what apply_triangulation calls; its SVD is of A, ours the
 * eigen-decomposition of A^T A, as the reference's own _triangulatePy).  tests/track_oracle.py restates every expression
 * in the same order in numpy and the kernels equal it bit for bit; tests/golden/track_golden.npz holds what the
 * reference's _triangulatePy and project give on the same inputs.
 *
 * Every NaN this ABI writes is the one quiet NaN 0x7ff8000000000000.  All arithmetic is fp64 with + - x / sqrt only,
 * compiled without FMA contraction; there are no floating-point atomics: two runs are bitwise equal.
 *
 * Launch chain of trk_update (three launches, no host round trip): one workgroup compacts and classifies
 * (wg::excl_scan) | one thread per pair across the device does the projections and the DLT | one workgroup does the
 * median, the gate, the candidate scan, the ids and the unmatched list.
 *
 * Conventions as in mapping.h: device pointers, caller-provided workspace (256-byte aligned), work enqueued on `stream`,
 * no allocation, no synchronisation, 0 = OK / negative = error (-1 bad argument, -2 workspace too small, -3 launch
 * failed) + map_last_error().
 */
#ifndef ONEPOSE_AMD_TRACK_UPDATE_H
#define ONEPOSE_AMD_TRACK_UPDATE_H

#include "mapping.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRK_MAX_KEYPOINTS 8192 /* bounds n_kf, n_q and the n of the stage entries' single-workgroup kernels */
#define TRK_SUMMARY_ENTRIES 8  /* m, known, known kept, candidates, candidates kept, non-finite removed, ignored, unmatched */

/* Bytes of workspace trk_update takes for n_kf keyframe and n_q query keypoints; 0 = refused (either outside
 * [1, TRK_MAX_KEYPOINTS]). */
size_t trk_workspace_bytes(int n_kf, int n_q);

/* The whole step.  Inputs: matches0 [n_kf] (query index or -1), kf_xy [n_kf][2], q_xy [n_q][2] fp32, kf_pt_ids [n_kf]
 * (-1 or a row of points), points [n_points][3] (n_points >= 0; may be NULL when it is 0), K_kf, K_q [3][3], pose_kf,
 * pose_q [4][4] row-major world -> camera (only the top three rows are read), all on the device; gate_factor,
 * max_reproj, max_z finite and positive (the reference: 1.2, 20, 0.15).
 * Outputs: pair_kf, pair_q, q_pt_ids [n_kf] (rows >= m: -1); pair_dist [n_kf][2] (known: d, NaN; candidate: rep_q,
 * rep_kf; ignored id: NaN, NaN; rows >= m: NaN); new_points [n_kf][3] (rows past the kept count are not written);
 * unmatched_q [n_q] (rows past the count: -1); median [1] = med; summary [TRK_SUMMARY_ENTRIES] int32.  m == 0 is valid. */
int trk_update(const int32_t* matches0, const float* kf_xy, const float* q_xy, const int32_t* kf_pt_ids, const double* points,
               const double* K_kf, const double* K_q, const double* pose_kf, const double* pose_q, int n_kf, int n_q, int n_points,
               double gate_factor, double max_reproj, double max_z, int32_t* pair_kf, int32_t* pair_q, int32_t* q_pt_ids,
               double* pair_dist, double* new_points, int32_t* unmatched_q, double* median, int32_t* summary, void* workspace,
               size_t workspace_bytes, map_stream_t stream);

/* Stage: the two-view DLT of step 4 alone, on the same device function.  P1, P2 [3][4] row-major (device), xy1, xy2
 * [n][2] fp32, X [n][3]; n >= 1. */
int trk_triangulate_pairs(const double* P1, const double* P2, const float* xy1, const float* xy2, int n, double* X, map_stream_t stream);

/* Stage: the exact median and the gate of step 3.  dist [n], n in [1, TRK_MAX_KEYPOINTS], factor finite and positive ->
 * median [1] = factor x numpy.median(dist), keep [n] = dist < median[0].  The workspace is that of
 * trk_workspace_bytes(n, 1); the selection as built keeps its keys in registers and does not touch it. */
int trk_gate_median(const double* dist, int n, double factor, double* median, int32_t* keep, void* workspace, size_t workspace_bytes,
                    map_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
