/*
 * C ABI of the MI355X (gfx950) flow step of the keyframe tracker -- what OnePose's BATracker
 * (src/tracker/ba_tracker.py:113-126, 295-356) does to give a tracked frame its initial pose:
 * cv2.calcOpticalFlowPyrLK(winSize = (15, 15), maxLevel = 2, criteria = (EPS | COUNT, 10, 0.03)) from the
 * keyframe's crop into the new one, then PnP on the survivors (pnp.h) and the mean reprojection distance.
 * A second header of libdet_hip.so (det_version() 2); errors are read with det_last_error().
 *
 * The algorithm is the published pyramidal Lucas-Kanade (Bouguet) in OpenCV's fixed-point arrangement.
 * Everything that touches pixels is integer arithmetic, so the sums are exact and independent of their
 * order; the per-point algebra is fp64, one correctly rounded + - * / sqrt floor rint at a time
 * (tests/flow_oracle.py restates it and is compared bit for bit):
 *   images   uint8 [H][W]; I(x, y) outside the image is BORDER_REFLECT_101 (-1 -> 1, W -> W - 2).
 *   pyramid  level l + 1 is ((W_l + 1) / 2) x ((H_l + 1) / 2):
 *            out(x, y) = (sum_{i,j = 0..4} k_i k_j I_l(2x + i - 2, 2y + j - 2) + 128) >> 8, k = [1 4 6 4 1].
 *            The top level L is the largest l <= max_level with every level 1..l wider than win_w and
 *            higher than win_h.
 *   Scharr   Ix = 3 (I(x+1,y-1) - I(x-1,y-1)) + 10 (I(x+1,y) - I(x-1,y)) + 3 (I(x+1,y+1) - I(x-1,y+1)),
 *            Iy its transpose, neighbours reflected; Ix = Iy = 0 at a pixel outside the level.
 *   weights  at a fractional offset (a, b): w00 = rint((1-a)(1-b) 16384), w01 = rint(a (1-b) 16384),
 *            w10 = rint((1-a) b 16384), w11 = 16384 - w00 - w01 - w10 (rint: half to even, on doubles).
 *   samples  patch(F, X, Y) = F(X,Y) w00 + F(X+1,Y) w01 + F(X,Y+1) w10 + F(X+1,Y+1) w11; an image value is
 *            (patch + 256) >> 9 (5 fractional bits), a derivative value (patch + 8192) >> 14; arithmetic shifts.
 *   a point  p is fp32, widened; half = ((win_w - 1) / 2, (win_h - 1) / 2).  For l = L .. 0:
 *            1. prev = p 2^-l.
 *            2. at l = L next = prev (or guess 2^-L when an initial guess is given); below, next = 2 next.
 *            3. c = prev - half, ip = floor(c), (a, b) = c - ip.
 *            4. range test: ip.x < -win_w, ip.x >= W_l, ip.y < -win_h or ip.y >= H_l fails: status = 0 when
 *               l = 0, the level is skipped (next is carried down).
 *            5. ival, ix, iy over the win_w x win_h samples from ip; A11 = sum ix^2, A12 = sum ix iy,
 *               A22 = sum iy^2 (int64); a11 = A11 2^-20, a12, a22 alike; D = a11 a22 - a12 a12;
 *               minEig = (a22 + a11 - sqrt((a11 - a22)(a11 - a22) + 4 a12 a12)) / (2 win_w win_h).
 *            6. minEig < min_eig_threshold or D < 2^-23: status = 0 when l = 0, the level is skipped.
 *            7. j = 0 .. max_iter - 1, pd = 0: c = next - half, in = floor(c), the range test (failure:
 *               status = 0 when l = 0, leave the loop); weights from c - in, jval over the window of the
 *               second image; B1 = sum (jval - ival) ix, B2 = sum (jval - ival) iy (int64), b = B 2^-20;
 *               d = ((a12 b2 - a22 b1) / D, (a12 b1 - a11 b2) / D); next += d;
 *               stop if dx dx + dy dy <= eps eps; if j > 0, |dx + pdx| < 0.01 and |dy + pdy| < 0.01:
 *               next -= 0.5 d and stop; pd = d.
 *            8. after level 0, a status still 1 takes the range test once more on floor(next - half).
 *   outputs  next rounded to fp32 (the last estimate, whatever the status), status, and
 *            matches0[i] = status ? i : -1 -- the form pnp_ransac_epnp_matches reads, so the survivors go to
 *            the pose solver without a compaction on the host.  cv2's `err` output is not produced (the
 *            reference ignores it).
 * NOT claimed: parity with cv2.calcOpticalFlowPyrLK itself.  OpenCV keeps the points and the 2x2 algebra in
 * fp32, accumulates A and b in fp32 in SIMD order, and its border and final-status details vary by version.
 * Nobody has measured those differences here (no cv2 on the development machines); tests/test_flow_cv2.py
 * records them where cv2 exists.
 *
 * Conventions as in detector.h / pnp.h: device pointers, caller-provided workspace, work enqueued on
 * `stream`, no allocation, no synchronisation, 0 = OK / non-zero = error + det_last_error().
 */
#ifndef ONEPOSE_AMD_FLOW_H
#define ONEPOSE_AMD_FLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* flow_stream_t; /* hipStream_t */

#define FLOW_MIN_WINDOW 3 /* win_w, win_h: odd, in [3, 31] */
#define FLOW_MAX_WINDOW 31
#define FLOW_MAX_LEVEL 5 /* max_level in [0, 5]: at most 6 levels */
#define FLOW_MAX_ITERATIONS 100
#define FLOW_MAX_SIZE 4096 /* H, W in [2, 4096] */
#define FLOW_MAX_POINTS 65536
#define FLOW_REGISTER_SAMPLES 256 /* windows of at most this many samples keep their patches in registers */
#define FLOW_REPROJ_THREADS 256   /* the reduction order of flow_reproj_mean */
/* trace exit codes */
#define FLOW_EXIT_CONVERGED 0     /* |d|^2 <= eps^2 */
#define FLOW_EXIT_OSCILLATION 1   /* d + previous d below 0.01 on both axes */
#define FLOW_EXIT_ITERATION_CAP 2 /* max_iter iterations run */
#define FLOW_EXIT_LEFT_RANGE 3    /* the window of `next` left the level */
#define FLOW_EXIT_REJECTED 4      /* minEig or D below its threshold: no iteration */
#define FLOW_EXIT_SKIPPED 5       /* the window of `prev` failed the first range test */

/* Host-only.  bytes of the packed pyramid of an H x W image with max_level + 1 levels (level after level, rows
 * dense); 0 = refused. */
size_t flow_pyramid_bytes(int H, int W, int max_level);
/* number of levels L + 1 the tracker uses for this window (see `pyramid` above); 0 = refused. */
int flow_pyramid_levels(int H, int W, int win_w, int win_h, int max_level);
/* bytes of workspace of flow_track for n points: windows above FLOW_REGISTER_SAMPLES samples keep the int16
 * ival / ix / iy patches of the level at hand there; 0 = refused. */
size_t flow_workspace_bytes(int n, int win_w, int win_h);

/* Packs `levels` levels into `pyramid` (flow_pyramid_bytes(H, W, levels - 1) bytes), one launch per level.
 * Level 0 is a copy of image_u8; image_u8 == pyramid (level 0 already in place) enqueues no copy.  The
 * keyframe's pyramid is built once and reused for every frame tracked against it. */
int flow_build_pyramid(const uint8_t* image_u8, int H, int W, int levels, uint8_t* pyramid, flow_stream_t stream);

/* Stage entry on the tracker's device functions: steps 3-5 at given positions of one level.
 *   pts64 [n][2] double: `prev` in that level's coordinates; out_sums [n][3] int64 = {A11, A12, A22};
 *   out_patches [n][3][win_h win_w] int16 = the ival, ix, iy samples, row-major over the window.
 *   A position that fails the range test gives zeros. */
int flow_patch_sums(const uint8_t* pyramid, int H, int W, int level, const double* pts64, int n, int win_w, int win_h,
                    int64_t* out_sums, int16_t* out_patches, flow_stream_t stream);

/* Stage entry: {B1, B2} of step 7 for one given pair of positions per point (prev64, next64 [n][2] double, in the
 * level's coordinates); out_sums [n][2] int64, zeros when either position fails the range test. */
int flow_mismatch_sums(const uint8_t* pyramid_i, const uint8_t* pyramid_j, int H, int W, int level, const double* prev64,
                       const double* next64, int n, int win_w, int win_h, int64_t* out_sums, flow_stream_t stream);

/* The tracker: all levels of all points in one launch.
 *   pyramid_i, pyramid_j: `levels` packed levels of the first and second H x W image;
 *   pts [n][2] fp32; init [n][2] fp32 or null; next_pts [n][2] fp32; status [n] int32; matches0 [n] int64;
 *   trace [n][levels][2] int32 or null: per point and level {iterations run, exit code (FLOW_EXIT_*)}.
 *   n = 0 enqueues nothing.  workspace: flow_workspace_bytes(n, win_w, win_h) bytes, 256-byte aligned. */
int flow_track(const uint8_t* pyramid_i, const uint8_t* pyramid_j, int H, int W, int levels, const float* pts, const float* init, int n,
               int win_w, int win_h, int max_iter, double eps, double min_eig_threshold, float* next_pts, int32_t* status,
               int64_t* matches0, int32_t* trace, void* workspace, size_t workspace_bytes, flow_stream_t stream);

/* mean || project(X, K, pose) - x || over the points with status == 1 (ba_tracker.py:326-327; tracking_utils.project:
 * c = R X + t, h = K c, (h0 / h2, h1 / h2)), in fp64 on the fp32 points.
 *   pose [3][4] double (device, as pnp.h writes it); K_host: 9 doubles on the HOST, row-major;
 *   pts3d [n][3], pts2d [n][2] fp32; status [n] int32; out [2] double (device) = {mean (NaN when none), count}.
 * One workgroup, fixed-order reduction: two runs are bitwise equal. */
int flow_reproj_mean(const double* pose, const double* K_host, const float* pts3d, const float* pts2d, const int32_t* status, int n,
                     double* out, flow_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
