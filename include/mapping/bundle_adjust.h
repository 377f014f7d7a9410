/*
 * C ABI of the MI355X (gfx950) windowed bundle adjustment, part of libmap_hip.so (map_version() >= 2).
 *
 * Replaces, on the GPU, the numerical core of the reference's keyframe tracker,
 *   src/tracker/ba_tracker.py:358-441  (BATracker.apply_ba)
 * a Levenberg-Marquardt bundle adjustment over the keyframes of a sliding window and the 3D points they see, on the
 * residual of src/tracker/tracking_utils.py:91-169 (AngleAxisRotatePoint, SnavelyReprojectionErrorV2).
 *
 * The reference hands the optimisation to DeepLM, a third-party CUDA library that is neither vendored by the reference
 * nor installed here.  The algorithm below is OURS, not DeepLM's: the published Ceres-style trust-region LM on the exact
 * Schur complement.
 *   - damped system (H + D^2 / mu) delta = -g, H = J^T J, g = J^T r, D^2 = clamp(diag H, 1e-6, 1e32); mu starts at 1e4;
 *   - cost = 1/2 sum r^2; model decrease = -(delta^T g + 1/2 delta^T H delta), summed observation by observation as
 *     -(r . J delta + 1/2 |J delta|^2); rho = (cost - candidate cost) / model decrease;
 *   - a step is accepted when the candidate cost is finite, the model decrease is positive (as in Ceres; it is
 *     whenever the factorisation succeeds, up to rounding) and rho > 1e-3;
 *   - accepted: mu <- min(mu / max(1/3, 1 - (2 rho - 1)^3), 1e16), nu <- 2;  rejected: mu <- mu / nu, nu <- 2 nu;
 *   - num_iterations steps are attempted; the solve stops after num_success_iterations accepted ones (the reference
 *     passes 5 and 5);
 *   - a start whose cost is not finite changes nothing (status BA_STATUS_NONFINITE_START).
 * Linear solve: every point's 3x3 block V_j + D^2 / mu is inverted in closed form, the reduced camera system
 * S = U + D^2 / mu - sum_j W_j V_j^-1 W_j^T (order 6 C <= 192) is factorised by Cholesky in one workgroup (packed lower
 * triangle in LDS), the points follow by back-substitution.  A pivot that is not positive rejects the step.
 * NOT claimed: parity with DeepLM.  Known differences: DeepLM solves the normal equations by preconditioned conjugate
 * gradients, not exactly; it has its own damping and acceptance schedule.  Nobody has measured the difference: the
 * library is not here.  What IS pinned: residual and Jacobian against the reference's own residual function under
 * autograd (tests/golden/ba_residual_golden.npz), everything above against tests/ba_oracle.py.
 *
 * Residual, as the reference writes it: p' = AngleAxisRotatePoint(w, p) with its theta2 > 0 branch; at theta2 == 0 the
 * first-order form p + w x p IS the function and its Jacobian the Jacobian (what the reference's autograd gives: the
 * tracker starts from identity poses when PnP fails); then p' + t, division by the depth without a guard,
 * f x / z + c - observed.  fx and fy are separate here; with fx == fy the arithmetic is the reference's.  The rotation
 * derivative is a forward-mode dual through the same expression graph.  All arithmetic is fp64 without FMA contraction.
 *
 * Problem: cams [C][6] (in/out): angle-axis rotation then translation, world -> camera (the first six BAL numbers of
 * ba_tracker.py:459-466); intr [C][4]: fx, fy, cx, cy (constant); points [P][3] (in/out); observations obs_cam [M],
 * obs_pt [M] int32 and obs_xy [M][2] double, in any order; cam_fixed [C] / pt_fixed [P] int32 masks (non-zero = held
 * fixed), either may be NULL = none fixed (the reference).  A fixed variable and a variable without observation come
 * back bit for bit.  An observation whose camera or point index is out of range is ignored (checked on the device) and
 * counted in summary[4].
 *
 * Launch chain of ba_solve (no host round trip): the one-time stable counting sort of the observations by camera and
 * by point (radix 64 per pass, one workgroup, wg::excl_scan), then per iteration: linearise (one thread per
 * observation) | per-camera U, g_c, cost (one workgroup per camera: thread t sums observations t, t + BA_CAMERA_CHUNK, ..
 * of the camera's list in that order, then wg::tree_sum) | per-point V, g_p (one thread per point, input order) | Schur
 * partials (one workgroup per chunk of points, point after point) | fixed-order reduction of the partials | Cholesky and
 * camera step | per-point back-substitution | model decrease (one workgroup, strided over the point-sorted list + tree) |
 * candidate cost | decide (rho, mu update: on the device) | apply.  After the success count is reached the remaining
 * launches return at once on a device flag.  Every sum is a fixed-order sequential or tree sum; there are no floating-point atomics: two runs
 * on the same input are bitwise equal.
 *
 * Conventions as in mapping.h: device pointers, caller-provided workspace (256-byte aligned), work enqueued on `stream`,
 * no allocation, no synchronisation, 0 = OK / negative = error (-1 bad argument, -2 workspace too small, -3 launch
 * failed) + map_last_error().
 */
#ifndef ONEPOSE_AMD_BUNDLE_ADJUST_H
#define ONEPOSE_AMD_BUNDLE_ADJUST_H

#include "mapping.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BA_MAX_CAMERAS 32
#define BA_MAX_POINTS 32768
#define BA_MAX_OBSERVATIONS 262144
#define BA_MAX_ITERATIONS 1000
#define BA_CAMERA_CHUNK 256 /* threads of the per-camera kernels: observation k of a camera goes to thread k % this */
#define BA_TRACE_COLUMNS 6  /* cost, candidate cost, model decrease, rho, mu used, accepted (1 / 0; -1 = not attempted) */
#define BA_SUMMARY_ENTRIES 6 /* initial cost, final cost, accepted, attempted, ignored observations, status */
#define BA_STATUS_OK 0
#define BA_STATUS_NONFINITE_START 1

/* Bytes of workspace every entry point below takes for C cameras, P points, M observations; 0 = refused
 * (C in [1, BA_MAX_CAMERAS], P in [1, BA_MAX_POINTS], M in [1, BA_MAX_OBSERVATIONS]). */
size_t ba_workspace_bytes(int C, int P, int M);

/* The whole solve.  trace [num_iterations][BA_TRACE_COLUMNS] and summary [BA_SUMMARY_ENTRIES] double (device).
 * num_iterations in [1, BA_MAX_ITERATIONS], num_success_iterations >= 1. */
int ba_solve(double* cams, const double* intr, double* points, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
             const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P, int M, int num_iterations, int num_success_iterations,
             double* trace, double* summary, void* workspace, size_t workspace_bytes, map_stream_t stream);

/* Stages, on caller buffers: each enqueues the launches ba_solve uses for that stage (the two that read the sorted
 * observation lists enqueue the one-time sort first).
 *
 * r [M][2], Jc [M][2][6] (d r / d camera), Jp [M][2][3] (d r / d point); zeros for an ignored observation. */
int ba_linearize(const double* cams, const double* intr, const double* points, const int32_t* obs_cam, const int32_t* obs_pt,
                 const double* obs_xy, int C, int P, int M, double* r, double* Jc, double* Jp, map_stream_t stream);

/* U [C][6][6], V [P][3][3], g_c [C][6], g_p [P][3] (zeros for a fixed or unobserved variable) and cost_cam [C]: the
 * cost of every camera's observations; the cost is their sum in camera order. */
int ba_normal_blocks(const double* r, const double* Jc, const double* Jp, const int32_t* obs_cam, const int32_t* obs_pt,
                     const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P, int M, double* U, double* V, double* g_c,
                     double* g_p, double* cost_cam, void* workspace, size_t workspace_bytes, map_stream_t stream);

/* The damped step at mu > 0: delta_c [C][6], delta_p [P][3] (exactly 0 for a fixed or unobserved variable),
 * model_decrease [1]. */
int ba_step(const double* U, const double* V, const double* g_c, const double* g_p, const double* r, const double* Jc,
            const double* Jp, const int32_t* obs_cam, const int32_t* obs_pt, const int32_t* cam_fixed, const int32_t* pt_fixed, int C,
            int P, int M, double mu, double* delta_c, double* delta_p, double* model_decrease, void* workspace,
            size_t workspace_bytes, map_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
