// Small fp64 algebra shared by the geometry kernels (pnp_kernels.hip, detector/detector.hip, detector/flow.hip,
// mapping/track_update.hip).  Device code, included by .hip files directly and never through another header.
//
// The header takes the floating-point contraction setting of the file that includes it: `#pragma clang fp contract(off)` is
// lexical, so a file that sets it must include this header AFTER the pragma (the geometry files put the pragma above all of
// their project includes), and every function below, template or not, is then compiled without FMAs wherever it is
// instantiated.  A file without the pragma (pnp_kernels.hip) gets the default contraction.  Functions that contain a
// contractible a * b + c: jacobi_eig, project.  tri is integer arithmetic and K9 is data: the setting does not reach them.
#pragma once
#include <hip/hip_runtime.h>

namespace geom {

// a 3 x 3 intrinsic matrix, row-major, passed to a kernel by value
struct K9 {
    double k[9];
};

// index of element (i, j) of a symmetric N x N matrix stored as its upper triangle, row by row
template <int N>
__host__ __device__ constexpr int tri(int i, int j) {
    return i <= j ? i * N - i * (i - 1) / 2 + (j - i) : j * N - j * (j - 1) / 2 + (i - j);
}

// cyclic Jacobi for a symmetric N x N matrix held as its packed upper triangle S (N (N + 1) / 2 doubles: together with
// the N x N eigenvector matrix that is 444 registers for N = 12 instead of 576): on exit S[tri(i, i)] = eigenvalues,
// columns of V = eigenvectors.  The (p, q) sweep is fully unrolled, so every index is a compile-time constant and the
// matrices live in registers; the sweep loop is rolled and stops when the off-diagonal mass is below 1e-30 of the
// diagonal mass.  Numpy restatement for N = 4: tests/track_oracle.py:jacobi4.
template <int N>
__device__ __forceinline__ void jacobi_eig(double (&S)[N * (N + 1) / 2], double (&V)[N][N], int max_sweeps) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sw = 0; sw < max_sweeps; ++sw) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            diag += S[tri<N>(p, p)] * S[tri<N>(p, p)];
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += S[tri<N>(p, q)] * S[tri<N>(p, q)];
        }
        if (!(off > 1e-30 * diag)) break;
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = S[tri<N>(p, q)];
                if (apq != 0.0) {
                    const double theta = (S[tri<N>(q, q)] - S[tri<N>(p, p)]) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        if (k != p && k != q) {
                            const double akp = S[tri<N>(k, p)], akq = S[tri<N>(k, q)];
                            S[tri<N>(k, p)] = c * akp - s * akq;
                            S[tri<N>(k, q)] = s * akp + c * akq;
                        }
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = c * vkp - s * vkq;
                        V[k][q] = s * vkp + c * vkq;
                    }
                    S[tri<N>(p, p)] -= t * apq;
                    S[tri<N>(q, q)] += t * apq;
                    S[tri<N>(p, q)] = 0.0;
                }
            }
    }
}

// tracking_utils.py:74-88 on one point; pose: [4][4] row-major, top three rows; K: the full 3x3
__device__ __forceinline__ void project(const double (&X)[3], const double* __restrict__ K, const double* __restrict__ pose, double& x, double& y) {
    double c[3], h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = ((pose[4 * r] * X[0] + pose[4 * r + 1] * X[1]) + pose[4 * r + 2] * X[2]) + pose[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = (K[3 * r] * c[0] + K[3 * r + 1] * c[1]) + K[3 * r + 2] * c[2];
    x = h[0] / h[2];
    y = h[1] / h[2];
}

}  // namespace geom
