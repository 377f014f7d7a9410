// RANSAC-EPnP pose solver (C ABI: include/pnp.h with include/pnp_batch.h; reference call site: src/utils/eval_utils.py:18-42).
//
// fp64 throughout, like the reference's float64 cv2 call.  Latency-bound small dense algebra, not MFMA work.  Every kernel takes
// the frame from blockIdx.y: one chain of launches answers a batch of frames (pnp_ransac_epnp_batch), and the single-frame entry
// points launch a batch of one.  Per frame:
//   hyp_kernel    one thread per hypothesis: hash-sampled minimal set of 5 (sampling::distinct) -> EPnP -> [R | t]
//   score_kernel  one wave per hypothesis: squared reprojection error of every correspondence, ballot count
//   best_kernel   one workgroup: first arg-max of the inlier counts, inlier mask + ordered index list of the best model
//                 (wg::excl_scan per 1024 correspondences)
//   gather_matches_kernel  one workgroup: ordered compaction of the valid matches (wg::excl_scan), inlier mask zeroed
//   refit_kernel  one wave: EPnP over the inliers (point sums by butterfly reductions: every lane ends with the same
//                 bits, then runs the same dense stage), pose written as [R | t / scale]
// The EPnP steps follow OpenCV calib3d/epnp.cpp (see oracle/pnp_oracle.py for the restated algorithm and citations).
#include <hip/hip_runtime.h>
#include <string.h>

#include <type_traits>

#include "../../include/pnp.h"
#include "capi_common.h"
#include "geometry_math.h"
#include "ransac_sample.h"
#include "wg_primitives.h"

namespace pnp {

struct Cam {
    double fu, fv, uc, vc;
};
constexpr int MODEL_POINTS = 5;

// ---- small dense algebra ------------------------------------------------------------------------------
// Everything below is written so that every array index is a compile-time constant after unrolling: the matrices then
// live in registers.  (A first version with run-time indices kept them in scratch memory and one 5-point EPnP took
// 10 ms of serial scratch latency.)

using geom::jacobi_eig;   // geometry_math.h: packed-symmetric cyclic Jacobi, N = 3 and N = 12 here
using geom::tri;

// least squares min |A x - b| for a 6 x NC system by Householder QR
template <int NC>
__device__ __forceinline__ void lstsq6(double (&A)[6][NC], double (&b)[6], double (&x)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        double nrm = 0.0;
#pragma unroll
        for (int i = k; i < 6; ++i) nrm += A[i][k] * A[i][k];
        nrm = sqrt(nrm);
        const double alpha = A[k][k] > 0.0 ? -nrm : nrm;
        double v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = i < k ? 0.0 : A[i][k];
        v[k] -= alpha;
        double vv = 0.0;
#pragma unroll
        for (int i = k; i < 6; ++i) vv += v[i] * v[i];
        if (vv > 0.0) {
#pragma unroll
            for (int j = k; j < NC; ++j) {
                double d = 0.0;
#pragma unroll
                for (int i = k; i < 6; ++i) d += v[i] * A[i][j];
                d = 2.0 * d / vv;
#pragma unroll
                for (int i = k; i < 6; ++i) A[i][j] -= d * v[i];
            }
            double d = 0.0;
#pragma unroll
            for (int i = k; i < 6; ++i) d += v[i] * b[i];
            d = 2.0 * d / vv;
#pragma unroll
            for (int i = k; i < 6; ++i) b[i] -= d * v[i];
        }
    }
#pragma unroll
    for (int k = NC - 1; k >= 0; --k) {
        double s = b[k];
#pragma unroll
        for (int j = k + 1; j < NC; ++j) s -= A[k][j] * x[j];
        x[k] = s / A[k][k];
    }
}

// eigen-decomposition of a symmetric 3x3 with the eigenpairs sorted by DESCENDING eigenvalue: w[k], columns E[.][k]
__device__ __forceinline__ void eig3_desc(double (&S)[6], double (&w)[3], double (&E)[3][3]) {
    double V[3][3];
    jacobi_eig<3>(S, V, 16);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) E[i][k] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int rank = 0;                           // number of eigenvalues ordered before column c (ties: lower index first)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            rank += (S[tri<3>(j, j)] > S[tri<3>(c, c)]) || (S[tri<3>(j, j)] == S[tri<3>(c, c)] && j < c);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rank == k) {
                w[k] = S[tri<3>(c, c)];
#pragma unroll
                for (int i = 0; i < 3; ++i) E[i][k] = V[i][c];
            }
    }
}

// The frames U, Vs of the SVD of a 3x3 matrix M by one-sided Jacobi (Hestenes): the COLUMNS of A = M V are rotated against each other
// until they are orthogonal; their lengths are then the singular values, each to its own relative accuracy -- which the eigenvalues
// of M^T M do not have below 1e-8 of the largest.  Columns sorted by descending length (ties: lower index first).  U's first column
// is a column of A, the second is orthogonalised against it once more, the third is their cross product with the orientation of
// A's third column -- or, where that column is exactly zero (rank 2), the orientation that makes det(U Vs^T) = +1.
__device__ __forceinline__ void svd3_frames(const double (&M)[3][3], double (&U)[3][3], double (&Vs)[3][3]) {
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { A[i][j] = M[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sw = 0; sw < 12; ++sw) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double al = A[0][p] * A[0][p] + A[1][p] * A[1][p] + A[2][p] * A[2][p];
                const double be = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q];
                const double ga = A[0][p] * A[0][q] + A[1][p] * A[1][q] + A[2][p] * A[2][q];
                if (ga * ga > 1e-30 * al * be) {               // false for a NaN
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
                        A[i][p] = c * ap - sn * aq; A[i][q] = sn * ap + c * aq;
                        V[i][p] = c * vp - sn * vq; V[i][q] = sn * vp + c * vq;
                    }
                    rotated = true;
                }
            }
        if (!rotated) break;
    }
    double len2[3], As[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) len2[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) { As[i][k] = A[i][k]; Vs[i][k] = V[i][k]; }       // a NaN length ranks nowhere: kept in place
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) rank += (len2[j] > len2[c]) || (len2[j] == len2[c] && j < c);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rank == k) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { As[i][k] = A[i][c]; Vs[i][k] = V[i][c]; }
            }
    }
    const double n0 = sqrt(As[0][0] * As[0][0] + As[1][0] * As[1][0] + As[2][0] * As[2][0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][0] = As[i][0] / n0;
    const double d01 = U[0][0] * As[0][1] + U[1][0] * As[1][1] + U[2][0] * As[2][1];
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][1] = As[i][1] - d01 * U[i][0];
    const double n1 = sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][1] /= n1;
    const double w[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1], U[0][0] * U[1][1] - U[1][0] * U[0][1]};
    const double along = w[0] * As[0][2] + w[1] * As[1][2] + w[2] * As[2][2];
    const double detv = Vs[0][0] * (Vs[1][1] * Vs[2][2] - Vs[1][2] * Vs[2][1]) - Vs[0][1] * (Vs[1][0] * Vs[2][2] - Vs[1][2] * Vs[2][0]) +
                        Vs[0][2] * (Vs[1][0] * Vs[2][1] - Vs[1][1] * Vs[2][0]);
    const double sgn = along < 0.0 ? -1.0 : (along > 0.0 ? 1.0 : (detv < 0.0 ? -1.0 : 1.0));
#pragma unroll
    for (int i = 0; i < 3; ++i) U[i][2] = sgn * w[i];
}

// R = U V^T of the SVD of a 3x3 matrix (absolute orientation), reflection fixed as epnp.cpp does (third row negated)
__device__ __forceinline__ void procrustes_rotation(const double (&M)[3][3], double (&R)[3][3]) {
    double B[6], w[3], Vs[3][3], U[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) B[tri<3>(i, j)] = M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j];   // M^T M
    eig3_desc(B, w, Vs);
    const double s0 = sqrt(fmax(w[0], 0.0)), s2 = sqrt(fmax(w[2], 0.0));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double sk = sqrt(fmax(w[k], 0.0));
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i][k] = (M[i][0] * Vs[0][k] + M[i][1] * Vs[1][k] + M[i][2] * Vs[2][k]) / sk;
    }
    // U = M V / sigma from the eigenpairs of M^T M is the cheap way and is kept, bit for bit, wherever it is good: every all-inlier
    // sample and the refit of a solid object.  It squares the condition number: U is orthonormal only to about
    // eps (sigma_0 / sigma_k)^2, and a sigma_k below 1e-8 sigma_0 is rounding noise.  A minimal set with an outlier in it, a thin slab
    // (sigma_2 / sigma_0 = its eigenvalue ratio: 1e-10 at thickness 1e-5) or a rod make M that ill-conditioned.  The first version
    // completed a rank-2 U by a cross product WITHOUT looking at det(Vs) -- a thin slab whose noise eigenvalue rounded to <= 0 then
    // got a reflection, 'fixed' into a wrong rotation 16 .. 147 px off -- and rebuilt a non-orthonormal U by Gram-Schmidt, which is
    // a rotation but not the nearest one (rods: 1e-5 between scale 1 and scale 1000).  Where the Gram matrix of U is off by more
    // than 1e-13, or sigma_2 is not above 1e-12 sigma_0, both frames now come from the SVD of M itself.
    double dev = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b)
            dev = fmax(dev, fabs(U[0][a] * U[0][b] + U[1][a] * U[1][b] + U[2][a] * U[2][b] - (a == b ? 1.0 : 0.0)));
    if (!(s2 > 1e-12 * s0 && dev <= 1e-13)) svd3_frames(M, U, Vs);              // also taken for a NaN, which stays one
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = U[i][0] * Vs[j][0] + U[i][1] * Vs[j][1] + U[i][2] * Vs[j][2];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0.0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[2][j] = -R[2][j];
    }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o);   // butterfly: a + b == b + a, so every lane ends with the same bits
    return x;
}

// ---- EPnP ---------------------------------------------------------------------------------------------------
// NPTS > 0: the calling thread solves its own NPTS-point problem (point loops unrolled, get(i) with constant i).
// NPTS == 0: the 64 lanes of a wave share the point loops of ONE n-point problem (butterfly reductions) and all run the
// dense stage on identical data.  get(i, pw, uv): i-th correspondence (object point already scaled).
// Returns false if the pose is not finite.
template <int NPTS, class Get>
__device__ __forceinline__ bool epnp_solve(int n_rt, Get get, const Cam& cam, double (&Rout)[3][3], double (&tout)[3]) {
    constexpr bool WAVE = NPTS == 0;
    const int n = WAVE ? n_rt : NPTS;
    const int lane = WAVE ? (threadIdx.x & 63) : 0;
    auto red = [](double x) { return WAVE ? wave_sum(x) : x; };
    // for_points(f): f(i) over this lane's share of the correspondences
    auto for_points = [&](auto f) {
        if constexpr (WAVE) {
            for (int i = lane; i < n; i += 64) f(i);
        } else {
#pragma unroll
            for (int i = 0; i < NPTS; ++i) f(i);
        }
    };
    // control points: centroid + sqrt(eigenvalue / n) * principal directions (choose_control_points)
    double c0[3] = {0, 0, 0};
    for_points([&](int i) {
        double pw[3], uv[2];
        get(i, pw, uv);
        c0[0] += pw[0]; c0[1] += pw[1]; c0[2] += pw[2];
    });
#pragma unroll
    for (int k = 0; k < 3; ++k) c0[k] = red(c0[k]) / n;
    double cov[6] = {};
    for_points([&](int i) {
        double pw[3], uv[2];
        get(i, pw, uv);
        const double d[3] = {pw[0] - c0[0], pw[1] - c0[1], pw[2] - c0[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) cov[tri<3>(a, b)] += d[a] * d[b];
    });
#pragma unroll
    for (int k = 0; k < 6; ++k) cov[k] = red(cov[k]);
    double w3[3], EV[3][3];
    eig3_desc(cov, w3, EV);
    // a flat set gets no pose (pnp.h): below PNP_FLATNESS_TAU the fourth control point sits on the first to rounding, CC is
    // singular and what follows is NaN or a finite wrong pose as rounding has it.  False for a NaN and for an all-zero covariance.
    if (!(w3[2] > PNP_FLATNESS_TAU * w3[0])) return false;
    double cws[4][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cws[0][k] = c0[k];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        // canonical eigenvector sign (largest-magnitude component positive, first on ties): with noisy data the solution
        // depends at noise level on which of the two mirrored control points is used
        const double a0 = fabs(EV[0][j]), a1 = fabs(EV[1][j]), a2 = fabs(EV[2][j]);
        const double lead = (a0 >= a1 && a0 >= a2) ? EV[0][j] : (a1 >= a2 ? EV[1][j] : EV[2][j]);
        const double kk = (lead < 0.0 ? -1.0 : 1.0) * sqrt(fmax(w3[j], 0.0) / n);
#pragma unroll
        for (int k = 0; k < 3; ++k) cws[j + 1][k] = c0[k] + kk * EV[k][j];
    }
    // barycentric coordinates: inverse of CC = [cws1 - cws0 | cws2 - cws0 | cws3 - cws0]
    double CC[3][3], CI[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) CC[k][j] = cws[j + 1][k] - cws[0][k];
    const double det = CC[0][0] * (CC[1][1] * CC[2][2] - CC[1][2] * CC[2][1]) - CC[0][1] * (CC[1][0] * CC[2][2] - CC[1][2] * CC[2][0]) +
                       CC[0][2] * (CC[1][0] * CC[2][1] - CC[1][1] * CC[2][0]);
    CI[0][0] = (CC[1][1] * CC[2][2] - CC[1][2] * CC[2][1]) / det; CI[0][1] = (CC[0][2] * CC[2][1] - CC[0][1] * CC[2][2]) / det;
    CI[0][2] = (CC[0][1] * CC[1][2] - CC[0][2] * CC[1][1]) / det; CI[1][0] = (CC[1][2] * CC[2][0] - CC[1][0] * CC[2][2]) / det;
    CI[1][1] = (CC[0][0] * CC[2][2] - CC[0][2] * CC[2][0]) / det; CI[1][2] = (CC[0][2] * CC[1][0] - CC[0][0] * CC[1][2]) / det;
    CI[2][0] = (CC[1][0] * CC[2][1] - CC[1][1] * CC[2][0]) / det; CI[2][1] = (CC[0][1] * CC[2][0] - CC[0][0] * CC[2][1]) / det;
    CI[2][2] = (CC[0][0] * CC[1][1] - CC[0][1] * CC[1][0]) / det;
    auto alphas = [&](const double (&pw)[3], double (&a)[4]) {
        const double d[3] = {pw[0] - c0[0], pw[1] - c0[1], pw[2] - c0[2]};
#pragma unroll
        for (int j = 0; j < 3; ++j) a[j + 1] = CI[j][0] * d[0] + CI[j][1] * d[1] + CI[j][2] * d[2];
        a[0] = 1.0 - a[1] - a[2] - a[3];
    };
    // M^T M (fill_M), mean alphas, G_j = sum_i alpha_ij (pw_i - pw0)
    double A[78] = {};                      // M^T M, packed upper triangle
    double abar[4] = {0, 0, 0, 0}, G[4][3] = {};
    for_points([&](int i) {
        double pw[3], uv[2], a[4];
        get(i, pw, uv);
        alphas(pw, a);
        double r1[12], r2[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r1[3 * j] = a[j] * cam.fu; r1[3 * j + 1] = 0.0; r1[3 * j + 2] = a[j] * (cam.uc - uv[0]);
            r2[3 * j] = 0.0; r2[3 * j + 1] = a[j] * cam.fv; r2[3 * j + 2] = a[j] * (cam.vc - uv[1]);
            abar[j] += a[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) G[j][k] += a[j] * (pw[k] - c0[k]);
        }
#pragma unroll
        for (int p = 0; p < 12; ++p)
#pragma unroll
            for (int q = p; q < 12; ++q) A[tri<12>(p, q)] += r1[p] * r1[q] + r2[p] * r2[q];
    });
#pragma unroll
    for (int k = 0; k < 78; ++k) A[k] = red(A[k]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        abar[j] = red(abar[j]) / n;
#pragma unroll
        for (int k = 0; k < 3; ++k) G[j][k] = red(G[j][k]);
    }
    double afirst[4];
    {
        double pw[3], uv[2];
        get(0, pw, uv);
        alphas(pw, afirst);
    }
    // null space of M: the 4 eigenvectors of M^T M with the smallest eigenvalues (v[0] = smallest)
    double v[4][12];
    {
        double EV12[12][12];
        jacobi_eig<12>(A, EV12, 24);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int k = 0; k < 12; ++k) v[s][k] = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            int rank = 0;                       // eigenvalues ordered before column c (ascending, ties: lower index first)
#pragma unroll
            for (int j = 0; j < 12; ++j)
                rank += (A[tri<12>(j, j)] < A[tri<12>(c, c)]) || (A[tri<12>(j, j)] == A[tri<12>(c, c)] && j < c);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (rank == s) {
#pragma unroll
                    for (int k = 0; k < 12; ++k) v[s][k] = EV12[k][c];
                }
        }
    }
    // L (6 x 10) and rho (compute_L_6x10, compute_rho)
    constexpr int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {1, 2, 3, 2, 3, 3};
    double L[6][10], rho[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double dv[4][3];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int k = 0; k < 3; ++k) dv[s][k] = v[s][3 * PA[r] + k] - v[s][3 * PB[r] + k];
        auto dot = [&](int i, int j) { return dv[i][0] * dv[j][0] + dv[i][1] * dv[j][1] + dv[i][2] * dv[j][2]; };
        L[r][0] = dot(0, 0); L[r][1] = 2 * dot(0, 1); L[r][2] = dot(1, 1); L[r][3] = 2 * dot(0, 2); L[r][4] = 2 * dot(1, 2);
        L[r][5] = dot(2, 2); L[r][6] = 2 * dot(0, 3); L[r][7] = 2 * dot(1, 3); L[r][8] = 2 * dot(2, 3); L[r][9] = dot(3, 3);
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) d2 += (cws[PA[r]][k] - cws[PB[r]][k]) * (cws[PA[r]][k] - cws[PB[r]][k]);
        rho[r] = d2;
    }
    // three beta approximations, 5 Gauss-Newton steps each, pose of each, smallest reprojection error wins
    double Rc[3][3][3], tc[3][3];
    auto candidate = [&](auto NA, double (&Rk)[3][3], double (&tk)[3]) {
        constexpr int na = decltype(NA)::value;
        double b[4] = {0, 0, 0, 0};
        if constexpr (na == 0) {                                  // unknowns B11 B12 B13 B14
            double Aq[6][4], bq[6], x[4];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                Aq[r][0] = L[r][0]; Aq[r][1] = L[r][1]; Aq[r][2] = L[r][3]; Aq[r][3] = L[r][6];
                bq[r] = rho[r];
            }
            lstsq6<4>(Aq, bq, x);
            if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = -x[1] / b[0]; b[2] = -x[2] / b[0]; b[3] = -x[3] / b[0]; }
            else { b[0] = sqrt(x[0]); b[1] = x[1] / b[0]; b[2] = x[2] / b[0]; b[3] = x[3] / b[0]; }
        } else if constexpr (na == 1) {                           // B11 B12 B22
            double Aq[6][3], bq[6], x[3];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                Aq[r][0] = L[r][0]; Aq[r][1] = L[r][1]; Aq[r][2] = L[r][2];
                bq[r] = rho[r];
            }
            lstsq6<3>(Aq, bq, x);
            if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
            else { b[0] = sqrt(x[0]); b[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) b[0] = -b[0];
        } else {                                                  // B11 B12 B22 B13 B23
            double Aq[6][5], bq[6], x[5];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
#pragma unroll
                for (int c = 0; c < 5; ++c) Aq[r][c] = L[r][c];
                bq[r] = rho[r];
            }
            lstsq6<5>(Aq, bq, x);
            if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
            else { b[0] = sqrt(x[0]); b[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
            if (x[1] < 0) b[0] = -b[0];
            b[2] = x[3] / b[0];
        }
        for (int it = 0; it < 5; ++it) {                          // gauss_newton
            double Aq[6][4], bq[6], x[4];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double* l = L[r];
                Aq[r][0] = 2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3];
                Aq[r][1] = l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3];
                Aq[r][2] = l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3];
                Aq[r][3] = l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3];
                bq[r] = rho[r] - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2] +
                                  l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3]);
            }
            lstsq6<4>(Aq, bq, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] += x[k];
        }
        // compute_ccs / solve_for_sign / estimate_R_and_t
        double ccs[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) ccs[j][k] = b[0] * v[0][3 * j + k] + b[1] * v[1][3 * j + k] + b[2] * v[2][3 * j + k] + b[3] * v[3][3 * j + k];
        const double z0 = afirst[0] * ccs[0][2] + afirst[1] * ccs[1][2] + afirst[2] * ccs[2][2] + afirst[3] * ccs[3][2];
        const double sg = z0 < 0.0 ? -1.0 : 1.0;
        double pc0[3], ABt[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) pc0[k] = sg * (abar[0] * ccs[0][k] + abar[1] * ccs[1][k] + abar[2] * ccs[2][k] + abar[3] * ccs[3][k]);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) ABt[r][c] = sg * (ccs[0][r] * G[0][c] + ccs[1][r] * G[1][c] + ccs[2][r] * G[2][c] + ccs[3][r] * G[3][c]);
        procrustes_rotation(ABt, Rk);
#pragma unroll
        for (int r = 0; r < 3; ++r) tk[r] = pc0[r] - (Rk[r][0] * c0[0] + Rk[r][1] * c0[1] + Rk[r][2] * c0[2]);
    };
    candidate(std::integral_constant<int, 0>{}, Rc[0], tc[0]);
    candidate(std::integral_constant<int, 1>{}, Rc[1], tc[1]);
    candidate(std::integral_constant<int, 2>{}, Rc[2], tc[2]);
    double err[3] = {0, 0, 0};
    for_points([&](int i) {
        double pw[3], uv[2];
        get(i, pw, uv);
#pragma unroll
        for (int na = 0; na < 3; ++na) {
            const double X = Rc[na][0][0] * pw[0] + Rc[na][0][1] * pw[1] + Rc[na][0][2] * pw[2] + tc[na][0];
            const double Y = Rc[na][1][0] * pw[0] + Rc[na][1][1] * pw[1] + Rc[na][1][2] * pw[2] + tc[na][1];
            const double Z = Rc[na][2][0] * pw[0] + Rc[na][2][1] * pw[1] + Rc[na][2][2] * pw[2] + tc[na][2];
            const double du = uv[0] - (cam.uc + cam.fu * X / Z), dvv = uv[1] - (cam.vc + cam.fv * Y / Z);
            err[na] += sqrt(du * du + dvv * dvv);
        }
    });
#pragma unroll
    for (int na = 0; na < 3; ++na) err[na] = red(err[na]);
    // smallest finite error, first on ties (N = 1, 2, 3 order)
    const bool f0 = isfinite(err[0]), f1 = isfinite(err[1]), f2 = isfinite(err[2]);
    if (!(f0 || f1 || f2)) return false;
    const bool pick1 = f1 && (!f0 || err[1] < err[0]);
    const double e01 = pick1 ? err[1] : err[0];
    const bool pick2 = f2 && (!(f0 || f1) || err[2] < e01);
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Rout[r][c] = pick2 ? Rc[2][r][c] : (pick1 ? Rc[1][r][c] : Rc[0][r][c]);
            fin &= isfinite(Rout[r][c]);
        }
        tout[r] = pick2 ? tc[2][r] : (pick1 ? tc[1][r] : tc[0][r]);
        fin &= isfinite(tout[r]);
    }
    return fin;
}

// ---- kernels --------------------------------------------------------------------------------------------------
// Every kernel serves a batch of frames, the frame being blockIdx.y; the single-frame entry points launch a batch of one, so a
// frame runs the same machine code alone and in a batch.  What differs from frame to frame travels BY VALUE in the kernel
// arguments (1.6 KB of the 4 KB there are); a frame's arrays are found by frame index x a stride that the shape alone fixes.
struct Frame {
    Cam cam;
    unsigned long long seed;
    int n;                                 // correspondences (query keypoints for gather_matches_kernel) of the frame
};
struct Batch {                             // the shape first, then the frames: a batch of one reads what it needs from the first 80 bytes
    size_t p3_stride, p2_stride;           // bytes from one frame's correspondences to the next frame's
    size_t ws_stride;                      // bytes from one frame's workspace slice to the next frame's
    int cap;                               // length of a frame's inlier-mask row: entries past n are written as 0
    Frame frame[PNP_MAX_ITEMS];
};
static_assert(sizeof(Batch) + 16 * sizeof(void*) + 64 <= 4096, "Batch must fit the kernel arguments");

template <class T>
__device__ __forceinline__ T* frame_of(T* p, size_t stride_bytes, int frame) {
    using Byte = std::conditional_t<std::is_const_v<T>, const char, char>;
    return p ? reinterpret_cast<T*>(reinterpret_cast<Byte*>(p) + stride_bytes * (size_t)frame) : nullptr;
}

// n_dev != nullptr: the number of correspondences is only known on the device (gather_matches_kernel; a workspace piece)
__global__ __launch_bounds__(64) void hyp_kernel(const float* __restrict__ p3_all, const float* __restrict__ p2_all,
                                                 const int* __restrict__ n_dev, double scale, Batch f, int iterations,
                                                 double* __restrict__ hyp_all) {
    const int h = blockIdx.x * 64 + threadIdx.x, frame = blockIdx.y;
    if (h >= iterations) return;
    const float* __restrict__ p3 = frame_of(p3_all, f.p3_stride, frame);
    const float* __restrict__ p2 = frame_of(p2_all, f.p2_stride, frame);
    double* __restrict__ hyp = frame_of(hyp_all, f.ws_stride, frame);
    const Cam cam = f.frame[frame].cam;
    const unsigned long long seed = f.frame[frame].seed;
    const int n = n_dev ? *frame_of(n_dev, f.ws_stride, frame) : f.frame[frame].n;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (n < MODEL_POINTS) {                                  // too few matches: no model (eval_utils.py:40-42)
        for (int k = 0; k < 12; ++k) hyp[(size_t)h * 12 + k] = nan;
        return;
    }
    int idx[MODEL_POINTS];
    sampling::distinct(seed, h, n, idx);
    double spw[MODEL_POINTS][3], suv[MODEL_POINTS][2];
    for (int k = 0; k < MODEL_POINTS; ++k) {
        for (int c = 0; c < 3; ++c) spw[k][c] = (double)p3[(size_t)idx[k] * 3 + c] * scale;
        suv[k][0] = (double)p2[(size_t)idx[k] * 2];
        suv[k][1] = (double)p2[(size_t)idx[k] * 2 + 1];
    }
    auto get = [&](int i, double (&pw)[3], double (&uv)[2]) {
        pw[0] = spw[i][0]; pw[1] = spw[i][1]; pw[2] = spw[i][2];
        uv[0] = suv[i][0]; uv[1] = suv[i][1];
    };
    double R[3][3], t[3];
    const bool ok = epnp_solve<MODEL_POINTS>(MODEL_POINTS, get, cam, R, t);
    double* o = hyp + (size_t)h * 12;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = ok ? R[r][c] : nan;
        o[r * 4 + 3] = ok ? t[r] : nan;
    }
}

__device__ __forceinline__ bool is_inlier(const double* __restrict__ P, const float* __restrict__ p3, const float* __restrict__ p2,
                                          int i, double scale, const Cam& cam, double thr2) {
    const double x = (double)p3[(size_t)i * 3] * scale, y = (double)p3[(size_t)i * 3 + 1] * scale, z = (double)p3[(size_t)i * 3 + 2] * scale;
    const double X = P[0] * x + P[1] * y + P[2] * z + P[3];
    const double Y = P[4] * x + P[5] * y + P[6] * z + P[7];
    const double Z = P[8] * x + P[9] * y + P[10] * z + P[11];
    const double du = (double)p2[(size_t)i * 2] - (cam.uc + cam.fu * X / Z), dv = (double)p2[(size_t)i * 2 + 1] - (cam.vc + cam.fv * Y / Z);
    return du * du + dv * dv <= thr2;      // false for NaN poses / points at infinity
}

__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ p3_all, const float* __restrict__ p2_all,
                                                    const int* __restrict__ n_dev, double scale, Batch f, double thr2, int iterations,
                                                    const double* __restrict__ hyp_all, int* __restrict__ counts_all) {
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, frame = blockIdx.y;
    if (h >= iterations) return;
    const float* __restrict__ p3 = frame_of(p3_all, f.p3_stride, frame);
    const float* __restrict__ p2 = frame_of(p2_all, f.p2_stride, frame);
    const double* __restrict__ hyp = frame_of(hyp_all, f.ws_stride, frame);
    int* __restrict__ counts = frame_of(counts_all, f.ws_stride, frame);
    const Cam cam = f.frame[frame].cam;
    const int n = n_dev ? *frame_of(n_dev, f.ws_stride, frame) : f.frame[frame].n;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = hyp[(size_t)h * 12 + k];
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n && is_inlier(P, p3, p2, i, scale, cam, thr2);
        cnt += __popcll(__ballot(in));
    }
    if (lane == 0) counts[h] = cnt;
}

// src != nullptr: correspondence i came from query keypoint src[i]; the inlier mask is indexed by query keypoint
// (pre-zeroed by gather_matches_kernel, its padding included).  src == nullptr: the mask's padding n .. cap is zeroed here.
__global__ __launch_bounds__(1024) void best_kernel(const float* __restrict__ p3_all, const float* __restrict__ p2_all,
                                                    const int* __restrict__ n_dev, double scale, Batch f, double thr2, int iterations,
                                                    const double* __restrict__ hyp_all, const int* __restrict__ counts_all,
                                                    const int* __restrict__ src_all, int32_t* __restrict__ mask_all,
                                                    int* __restrict__ inl_all, int32_t* __restrict__ info_all) {
    __shared__ int sc[1024], si[1024], wsum[16];
    const int tid = threadIdx.x, frame = blockIdx.y;
    const float* __restrict__ p3 = frame_of(p3_all, f.p3_stride, frame);
    const float* __restrict__ p2 = frame_of(p2_all, f.p2_stride, frame);
    const double* __restrict__ hyp = frame_of(hyp_all, f.ws_stride, frame);
    const int* __restrict__ counts = frame_of(counts_all, f.ws_stride, frame);
    const int* __restrict__ src = frame_of(src_all, f.ws_stride, frame);
    int* __restrict__ inl_idx = frame_of(inl_all, f.ws_stride, frame);
    int32_t* __restrict__ mask = mask_all + (size_t)frame * f.cap;
    int32_t* __restrict__ info = info_all + (size_t)frame * 4;
    const Cam cam = f.frame[frame].cam;
    const int n = n_dev ? *frame_of(n_dev, f.ws_stride, frame) : f.frame[frame].n;
    int bc = -1, bi = 0x7FFFFFFF;
    for (int h = tid; h < iterations; h += 1024) {
        const int c = counts[h];
        if (c > bc) { bc = c; bi = h; }                    // ascending h per thread: first maximum kept
    }
    sc[tid] = bc; si[tid] = bi;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s && (sc[tid + s] > sc[tid] || (sc[tid + s] == sc[tid] && si[tid + s] < si[tid]))) {
            sc[tid] = sc[tid + s]; si[tid] = si[tid + s];
        }
        __syncthreads();
    }
    const int best = si[0], bcount = sc[0];
    const bool ok = bcount >= MODEL_POINTS;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = ok ? hyp[(size_t)best * 12 + k] : 0.0;
    int run = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {                 // inlier mask + ordered index list
        const int i = i0 + tid;
        const int in = ok && i < n && is_inlier(P, p3, p2, i, scale, cam, thr2);
        if (i < n) mask[src ? src[i] : i] = in;
        int tot;
        const int pos = wg::excl_scan<1024>(in, wsum, tot);
        if (in) inl_idx[run + pos] = i;
        run += tot;
    }
    if (!src)
        for (int i = n + tid; i < f.cap; i += 1024) mask[i] = 0;
    if (tid == 0) {
        info[0] = ok; info[1] = ok ? run : 0; info[2] = ok ? best : -1; info[3] = bcount < 0 ? 0 : bcount;
    }
}

// inference.py:148-152 on the device: valid = matches0 > -1; mkpts2d = kpts2d[valid]; mkpts3d = kpts3d[matches0[valid]] --
// ordered compaction by one workgroup per frame; also zeroes the per-keypoint inlier mask (all f.cap entries of the row).
// Rows of f.cap query keypoints per frame; k3_stride: floats from one frame's database points to the next frame's (0: shared).
__global__ __launch_bounds__(1024) void gather_matches_kernel(const float* __restrict__ kpts2d_all, const float* __restrict__ kpts3d_all,
                                                              const long long* __restrict__ matches0_all, Batch f, size_t k3_stride,
                                                              float* __restrict__ p2_all, float* __restrict__ p3_all,
                                                              int* __restrict__ src_all, int* __restrict__ count_all,
                                                              int32_t* __restrict__ mask_all) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, frame = blockIdx.y;
    const int n1 = f.frame[frame].n;
    const float* __restrict__ kpts2d = kpts2d_all + (size_t)frame * f.cap * 2;
    const float* __restrict__ kpts3d = kpts3d_all + (size_t)frame * k3_stride;
    const long long* __restrict__ matches0 = matches0_all + (size_t)frame * f.cap;
    float* __restrict__ p2 = frame_of(p2_all, f.ws_stride, frame);
    float* __restrict__ p3 = frame_of(p3_all, f.ws_stride, frame);
    int* __restrict__ src = frame_of(src_all, f.ws_stride, frame);
    int* __restrict__ count = frame_of(count_all, f.ws_stride, frame);
    int32_t* __restrict__ mask = mask_all + (size_t)frame * f.cap;
    int run = 0;
    for (int i0 = 0; i0 < n1; i0 += 1024) {
        const int i = i0 + tid;
        const long long m = i < n1 ? matches0[i] : -1;
        const int valid = m > -1;
        if (i < n1) mask[i] = 0;
        int tot;
        const int pos = wg::excl_scan<1024>(valid, wsum, tot);
        if (valid) {
            const int o = run + pos;
            p2[(size_t)o * 2] = kpts2d[(size_t)i * 2];
            p2[(size_t)o * 2 + 1] = kpts2d[(size_t)i * 2 + 1];
            for (int c = 0; c < 3; ++c) p3[(size_t)o * 3 + c] = kpts3d[(size_t)m * 3 + c];
            src[o] = i;
        }
        run += tot;
    }
    for (int i = n1 + tid; i < f.cap; i += 1024) mask[i] = 0;
    if (tid == 0) *count = run;
}

// EPnP over the listed correspondences (idx == nullptr: all f.frame[frame].n); info != nullptr: RANSAC refit (count from info[1]).
// A refit that refuses leaves what a solve without a model leaves (pnp.h): the frame's mask row is zeroed again, all f.cap entries.
__global__ __launch_bounds__(64) void refit_kernel(const float* __restrict__ p3_all, const float* __restrict__ p2_all, double scale,
                                                   Batch f, const int* __restrict__ idx_all, int32_t* __restrict__ info_all,
                                                   int32_t* __restrict__ mask_all, double* __restrict__ pose_all) {
    const int lane = threadIdx.x, frame = blockIdx.y;
    const float* __restrict__ p3 = frame_of(p3_all, f.p3_stride, frame);
    const float* __restrict__ p2 = frame_of(p2_all, f.p2_stride, frame);
    const int* __restrict__ idx = frame_of(idx_all, f.ws_stride, frame);
    int32_t* __restrict__ info = info_all ? info_all + (size_t)frame * 4 : nullptr;
    double* __restrict__ pose = pose_all + (size_t)frame * 12;
    const Cam cam = f.frame[frame].cam;
    bool ok = true;
    int n = f.frame[frame].n;
    if (info) { ok = info[0] != 0; n = info[1]; }
    const bool had_model = info && ok;
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
    if (ok && n >= 4) {
        auto get = [&](int i, double (&pw)[3], double (&uv)[2]) {
            const int j = idx ? idx[i] : i;
            pw[0] = (double)p3[(size_t)j * 3] * scale; pw[1] = (double)p3[(size_t)j * 3 + 1] * scale; pw[2] = (double)p3[(size_t)j * 3 + 2] * scale;
            uv[0] = (double)p2[(size_t)j * 2]; uv[1] = (double)p2[(size_t)j * 2 + 1];
        };
        double Rs[3][3], ts[3];
        if (epnp_solve<0>(n, get, cam, Rs, ts)) {
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) R[r][c] = Rs[r][c];
                t[r] = ts[r] / scale;
            }
        } else ok = false;
    } else ok = false;
    if (lane == 0) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) pose[r * 4 + c] = R[r][c];
            pose[r * 4 + 3] = t[r];
        }
    }
    if (had_model && !ok) {                                // the selection found a model and the refit refused it (ok: the same in every lane)
        for (int i = lane; i < f.cap; i += 64) mask_all[(size_t)frame * f.cap + i] = 0;
        if (lane == 0) { info[0] = 0; info[1] = 0; info[2] = -1; }
    }
}

// One frame's slice of the workspace.  The batched entry points lay b slices of (cap, iterations) end to end: a slice's
// size, and so every frame's addresses, depend on the shape alone.
struct Workspace {
    double* hyp;
    int *counts, *inl, *src, *count;
    float *p2, *p3;
    size_t bytes;
};
inline Workspace carve(void* base, int n, int iterations) {
    Workspace w;
    capi::Bump a(base);
    w.hyp = a.take<double>(sizeof(double) * 12 * (size_t)iterations);
    w.counts = a.take<int>(sizeof(int) * (size_t)iterations);
    w.inl = a.take<int>(sizeof(int) * (size_t)n);
    w.src = a.take<int>(sizeof(int) * (size_t)n);
    w.count = a.take<int>(sizeof(int));
    w.p2 = a.take<float>(sizeof(float) * 2 * (size_t)n);
    w.p3 = a.take<float>(sizeof(float) * 3 * (size_t)n);
    w.bytes = a.off;
    return w;
}

}  // namespace pnp

using namespace pnp;
using namespace capi;

namespace {
Cam cam_of(const double* K) { return Cam{K[0], K[4], K[2], K[5]}; }

// the batch of one frame the single-frame entry points launch
Batch one_frame(const double* K, int n, uint64_t seed) {
    Batch f = {};
    f.frame[0] = Frame{cam_of(K), seed, n};
    f.cap = n;
    return f;
}

// hypotheses -> scores -> selection -> refit of every frame of f, over correspondences p3 / p2 (n_dev: their counts, when only
// the device knows them; src: the query keypoint of each, for the mask)
void launch_solve(const float* p3, const float* p2, const int* n_dev, const int* src, const Batch& f, int b, double scale,
                  double thr2, int iterations, const Workspace& w, double* pose, int32_t* mask, int32_t* info, hipStream_t s) {
    hipLaunchKernelGGL(hyp_kernel, dim3(ceil_div(iterations, 64), b), dim3(64), 0, s, p3, p2, n_dev, scale, f, iterations, w.hyp);
    hipLaunchKernelGGL(score_kernel, dim3(ceil_div(iterations, 4), b), dim3(256), 0, s, p3, p2, n_dev, scale, f, thr2, iterations, w.hyp,
                       w.counts);
    hipLaunchKernelGGL(best_kernel, dim3(1, b), dim3(1024), 0, s, p3, p2, n_dev, scale, f, thr2, iterations, w.hyp, w.counts, src, mask,
                       w.inl, info);
    hipLaunchKernelGGL(refit_kernel, dim3(1, b), dim3(64), 0, s, p3, p2, scale, f, (const int*)w.inl, info, mask, pose);
}

// what the two batched entry points check alike; 0 or the code to return
int check_batch(const double* K_host, const int32_t* n, const uint64_t* seeds, int b, int cap, double scale, double reproj_error,
                int iterations, const void* pose, const void* inlier_mask, const void* info, const char* cap_name) {
    if (b < 1 || b > PNP_MAX_ITEMS) return fail(-1, "b must be in [1, %d] (got %d)", PNP_MAX_ITEMS, b);
    if (cap < 1) return fail(-1, "%s must be >= 1 (got %d)", cap_name, cap);
    if (!K_host || !n || !seeds || !pose || !inlier_mask || !info) return fail(-1, "null argument");
    for (int i = 0; i < b; ++i)
        if (n[i] < 0 || n[i] > cap) return fail(-1, "frame %d: n = %d is outside [0, %s = %d]", i, n[i], cap_name, cap);
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0) || !(reproj_error > 0.0)) return fail(-1, "scale and reproj_error must be positive");
    return 0;
}

int check_batch_workspace(const void* workspace, size_t workspace_bytes, int b, int cap, int iterations) {
    if (!workspace) return fail(-1, "workspace is null");
    const size_t need = (size_t)b * carve(nullptr, cap, iterations).bytes;
    if (workspace_bytes < need) return fail(-2, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    return 0;
}

Batch batch_of(const double* K_host, const int32_t* n, const uint64_t* seeds, int b, int cap, size_t ws_stride) {
    Batch f = {};
    for (int i = 0; i < b; ++i) {
        f.frame[i] = Frame{cam_of(K_host + 9 * i), (unsigned long long)seeds[i], n[i]};
    }
    f.cap = cap;
    f.ws_stride = ws_stride;
    return f;
}
}  // namespace

extern "C" {

int pnp_version(void) { return 3; }
const char* pnp_last_error(void) { return g_err; }

size_t pnp_workspace_bytes(int n, int iterations) {
    if (n < 1 || iterations < 1) { fail(-1, "n and iterations must be >= 1"); return 0; }
    return carve(nullptr, n, iterations).bytes;
}

size_t pnp_batch_workspace_bytes(int b, int cap, int iterations) {
    if (b < 1 || b > PNP_MAX_ITEMS || cap < 1 || iterations < 1 || iterations > (1 << 24)) {
        fail(-1, "b must be in [1, %d], cap >= 1 and iterations in [1, 2^24]", PNP_MAX_ITEMS);
        return 0;
    }
    return (size_t)b * carve(nullptr, cap, iterations).bytes;
}

int pnp_ransac_epnp(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, double reproj_error,
                    int iterations, uint64_t seed, double* pose, int32_t* inlier_mask, int32_t* info, void* workspace,
                    size_t workspace_bytes, pnp_stream_t stream) {
    if (!pts_3d || !pts_2d || !K_host || !pose || !inlier_mask || !info || !workspace) return fail(-1, "null argument");
    if (n < MODEL_POINTS) return fail(-1, "solvePnPRansac with EPNP needs at least %d correspondences (got %d)", MODEL_POINTS, n);
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0) || !(reproj_error > 0.0)) return fail(-1, "scale and reproj_error must be positive");
    Workspace w = carve(workspace, n, iterations);
    if (workspace_bytes < w.bytes) return fail(-1, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    launch_solve(pts_3d, pts_2d, nullptr, nullptr, one_frame(K_host, n, seed), 1, scale, reproj_error * reproj_error, iterations, w,
                 pose, inlier_mask, info, reinterpret_cast<hipStream_t>(stream));
    return check_launch(-1, "pnp_ransac_epnp");
}

int pnp_ransac_epnp_batch(const float* pts_3d, const float* pts_2d, const double* K_host, const int32_t* n, const uint64_t* seeds,
                          int b, int cap, double scale, double reproj_error, int iterations, double* pose, int32_t* inlier_mask,
                          int32_t* info, void* workspace, size_t workspace_bytes, pnp_stream_t stream) {
    if (const int rc = check_batch(K_host, n, seeds, b, cap, scale, reproj_error, iterations, pose, inlier_mask, info, "cap")) return rc;
    if (!pts_3d || !pts_2d) return fail(-1, "null argument");
    if (const int rc = check_batch_workspace(workspace, workspace_bytes, b, cap, iterations)) return rc;
    Workspace w = carve(workspace, cap, iterations);
    Batch f = batch_of(K_host, n, seeds, b, cap, w.bytes);
    f.p3_stride = sizeof(float) * 3 * (size_t)cap;
    f.p2_stride = sizeof(float) * 2 * (size_t)cap;
    launch_solve(pts_3d, pts_2d, nullptr, nullptr, f, b, scale, reproj_error * reproj_error, iterations, w, pose, inlier_mask, info,
                 reinterpret_cast<hipStream_t>(stream));
    return check_launch(-1, "pnp_ransac_epnp_batch");
}

int pnp_ransac_epnp_matches(const float* kpts2d, const float* kpts3d, const int64_t* matches0, int n1, const double* K_host,
                            double scale, double reproj_error, int iterations, uint64_t seed, double* pose, int32_t* inlier_mask,
                            int32_t* info, void* workspace, size_t workspace_bytes, pnp_stream_t stream) {
    if (!kpts2d || !kpts3d || !matches0 || !K_host || !pose || !inlier_mask || !info || !workspace) return fail(-1, "null argument");
    if (n1 < 1) return fail(-1, "n1 must be >= 1");
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0) || !(reproj_error > 0.0)) return fail(-1, "scale and reproj_error must be positive");
    Workspace w = carve(workspace, n1, iterations);
    if (workspace_bytes < w.bytes) return fail(-1, "workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Batch f = one_frame(K_host, n1, seed);
    hipLaunchKernelGGL(gather_matches_kernel, dim3(1, 1), dim3(1024), 0, s, kpts2d, kpts3d, reinterpret_cast<const long long*>(matches0),
                       f, (size_t)0, w.p2, w.p3, w.src, w.count, inlier_mask);
    launch_solve(w.p3, w.p2, w.count, w.src, f, 1, scale, reproj_error * reproj_error, iterations, w, pose, inlier_mask, info, s);
    return check_launch(-1, "pnp_ransac_epnp_matches");
}

int pnp_ransac_epnp_matches_batch(const float* kpts2d, const float* kpts3d, const int64_t* matches0, const double* K_host,
                                  const int32_t* n1, const uint64_t* seeds, int b, int cap1, int n3, int shared3d, double scale,
                                  double reproj_error, int iterations, double* pose, int32_t* inlier_mask, int32_t* info,
                                  void* workspace, size_t workspace_bytes, pnp_stream_t stream) {
    if (const int rc = check_batch(K_host, n1, seeds, b, cap1, scale, reproj_error, iterations, pose, inlier_mask, info, "cap1")) return rc;
    if (!kpts2d || !kpts3d || !matches0) return fail(-1, "null argument");
    if (n3 < 1) return fail(-1, "n3 must be >= 1 (got %d)", n3);
    if (shared3d != 0 && shared3d != 1) return fail(-1, "shared3d must be 0 or 1 (got %d)", shared3d);
    if (const int rc = check_batch_workspace(workspace, workspace_bytes, b, cap1, iterations)) return rc;
    Workspace w = carve(workspace, cap1, iterations);
    Batch f = batch_of(K_host, n1, seeds, b, cap1, w.bytes);
    f.p3_stride = f.p2_stride = w.bytes;                  // the gathered correspondences are pieces of the workspace slices
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gather_matches_kernel, dim3(1, b), dim3(1024), 0, s, kpts2d, kpts3d, reinterpret_cast<const long long*>(matches0),
                       f, shared3d ? (size_t)0 : (size_t)3 * n3, w.p2, w.p3, w.src, w.count, inlier_mask);
    launch_solve(w.p3, w.p2, w.count, w.src, f, b, scale, reproj_error * reproj_error, iterations, w, pose, inlier_mask, info, s);
    return check_launch(-1, "pnp_ransac_epnp_matches_batch");
}

int pnp_epnp(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, double* pose, void* workspace,
             size_t workspace_bytes, pnp_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (!pts_3d || !pts_2d || !K_host || !pose) return fail(-1, "null argument");
    if (n < 4) return fail(-1, "EPnP needs at least 4 correspondences (got %d)", n);
    if (!(scale > 0.0)) return fail(-1, "scale must be positive");
    hipLaunchKernelGGL(refit_kernel, dim3(1, 1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), pts_3d, pts_2d, scale,
                       one_frame(K_host, n, 0), (const int*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, pose);
    return check_launch(-1, "pnp_epnp");
}

// ---- the stages of pnp_ransac_epnp on caller-provided buffers (stage tests): the same kernels, the same launch shapes ----
int pnp_hypotheses(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, int iterations,
                   uint64_t seed, double* hyp, pnp_stream_t stream) {
    if (!pts_3d || !pts_2d || !K_host || !hyp) return fail(-1, "null argument");
    if (n < MODEL_POINTS) return fail(-1, "solvePnPRansac with EPNP needs at least %d correspondences (got %d)", MODEL_POINTS, n);
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0)) return fail(-1, "scale must be positive");
    hipLaunchKernelGGL(hyp_kernel, dim3(ceil_div(iterations, 64), 1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), pts_3d, pts_2d,
                       (const int*)nullptr, scale, one_frame(K_host, n, seed), iterations, hyp);
    return check_launch(-1, "pnp_hypotheses");
}

int pnp_score_hypotheses(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, double reproj_error,
                         const double* hyp, int iterations, int32_t* counts, pnp_stream_t stream) {
    if (!pts_3d || !pts_2d || !K_host || !hyp || !counts) return fail(-1, "null argument");
    if (n < MODEL_POINTS) return fail(-1, "solvePnPRansac with EPNP needs at least %d correspondences (got %d)", MODEL_POINTS, n);
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0) || !(reproj_error > 0.0)) return fail(-1, "scale and reproj_error must be positive");
    hipLaunchKernelGGL(score_kernel, dim3(ceil_div(iterations, 4), 1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pts_3d, pts_2d,
                       (const int*)nullptr, scale, one_frame(K_host, n, 0), reproj_error * reproj_error, iterations, hyp, counts);
    return check_launch(-1, "pnp_score_hypotheses");
}

int pnp_select_best(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, double reproj_error,
                    const double* hyp, const int32_t* counts, int iterations, int32_t* inlier_mask, int32_t* inlier_idx,
                    int32_t* info, pnp_stream_t stream) {
    if (!pts_3d || !pts_2d || !K_host || !hyp || !counts || !inlier_mask || !inlier_idx || !info) return fail(-1, "null argument");
    if (n < MODEL_POINTS) return fail(-1, "solvePnPRansac with EPNP needs at least %d correspondences (got %d)", MODEL_POINTS, n);
    if (iterations < 1 || iterations > (1 << 24)) return fail(-1, "iterations out of range");
    if (!(scale > 0.0) || !(reproj_error > 0.0)) return fail(-1, "scale and reproj_error must be positive");
    hipLaunchKernelGGL(best_kernel, dim3(1, 1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), pts_3d, pts_2d, (const int*)nullptr,
                       scale, one_frame(K_host, n, 0), reproj_error * reproj_error, iterations, hyp, counts, (const int*)nullptr,
                       inlier_mask, inlier_idx, info);
    return check_launch(-1, "pnp_select_best");
}

int pnp_refit(const float* pts_3d, const float* pts_2d, const double* K_host, double scale, int n, const int32_t* inlier_idx,
              int32_t* inlier_mask, int32_t* info, double* pose, pnp_stream_t stream) {
    if (!pts_3d || !pts_2d || !K_host || !inlier_idx || !inlier_mask || !info || !pose) return fail(-1, "null argument");
    if (n < MODEL_POINTS) return fail(-1, "solvePnPRansac with EPNP needs at least %d correspondences (got %d)", MODEL_POINTS, n);
    if (!(scale > 0.0)) return fail(-1, "scale must be positive");
    hipLaunchKernelGGL(refit_kernel, dim3(1, 1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), pts_3d, pts_2d, scale,
                       one_frame(K_host, n, 0), (const int*)inlier_idx, info, inlier_mask, pose);
    return check_launch(-1, "pnp_refit");
}

}  // extern "C"
