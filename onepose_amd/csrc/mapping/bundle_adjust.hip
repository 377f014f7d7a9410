// Windowed bundle adjustment for gfx950: Levenberg-Marquardt on the exact Schur complement (include/mapping/bundle_adjust.h).
//
// A latency-bound chain of small fp64 kernels, like pnp_kernels.hip: no MFMA.  Every sum is sequential or a wg::tree_sum in
// a fixed order, no floating-point atomics.  tests/ba_oracle.py restates the arithmetic in numpy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#pragma clang fp contract(off)   // above every project include: a shared header takes the setting of the file that includes it

#include "../../../include/mapping/bundle_adjust.h"
#include "../capi_common.h"
#include "../wg_primitives.h"

namespace bak {

constexpr int CAM = 6, PT = 3;
constexpr int LIN_THREADS = 256;
constexpr int CAM_THREADS = BA_CAMERA_CHUNK;
constexpr int SORT_THREADS = 512, RADIX_BITS = 6, RADIX = 1 << RADIX_BITS;
constexpr int SCHUR_THREADS = 256, MAX_CHUNKS = 128, MIN_CHUNK_POINTS = 8;
constexpr int CHOL_THREADS = 1024;
constexpr int MODEL_THREADS = 1024;
constexpr double MU0 = 1e4, MU_MAX = 1e16, MIN_RHO = 1e-3, DIAG_MIN = 1e-6, DIAG_MAX = 1e32;

// state of one solve, on the device: written by ba_init_kernel, the Cholesky kernel (chol_fail) and ba_decide_kernel
struct Ctrl {
    double mu, nu, initial_cost, final_cost;
    int n_acc, n_att, done, accept, status, chol_fail;
};

__device__ __forceinline__ bool in_range(int c, int j, int C, int P) { return (unsigned)c < (unsigned)C && (unsigned)j < (unsigned)P; }
__device__ __forceinline__ bool finished(const Ctrl* ctrl) { return ctrl && ctrl->done; }
__device__ __forceinline__ double clamp_diag(double d) { return fmin(fmax(d, DIAG_MIN), DIAG_MAX); }

// ---- forward-mode dual over the three rotation parameters -------------------------------------------------------------------

struct D3 {
    double v, d[3];
};
__device__ __forceinline__ D3 operator+(const D3& a, const D3& b) { return {a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2]}}; }
__device__ __forceinline__ D3 operator-(const D3& a, const D3& b) { return {a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2]}}; }
__device__ __forceinline__ D3 operator*(const D3& a, const D3& b) {
    return {a.v * b.v, {a.d[0] * b.v + a.v * b.d[0], a.d[1] * b.v + a.v * b.d[1], a.d[2] * b.v + a.v * b.d[2]}};
}
__device__ __forceinline__ D3 operator*(const D3& a, double b) { return {a.v * b, {a.d[0] * b, a.d[1] * b, a.d[2] * b}}; }
__device__ __forceinline__ D3 operator+(double a, const D3& b) { return {a + b.v, {b.d[0], b.d[1], b.d[2]}}; }
__device__ __forceinline__ D3 operator-(double a, const D3& b) { return {a - b.v, {-b.d[0], -b.d[1], -b.d[2]}}; }
__device__ __forceinline__ double value(double a) { return a; }
__device__ __forceinline__ double value(const D3& a) { return a.v; }
__device__ __forceinline__ double t_sqrt(double a) { return sqrt(a); }
__device__ __forceinline__ D3 t_sqrt(const D3& a) {
    const double s = sqrt(a.v), k = 0.5 / s;
    return {s, {a.d[0] * k, a.d[1] * k, a.d[2] * k}};
}
__device__ __forceinline__ double t_recip(double a) { return 1.0 / a; }
__device__ __forceinline__ D3 t_recip(const D3& a) {
    const double i = 1.0 / a.v, k = -(i * i);
    return {i, {a.d[0] * k, a.d[1] * k, a.d[2] * k}};
}
__device__ __forceinline__ void t_sincos(double a, double& s, double& c) { s = sin(a); c = cos(a); }
__device__ __forceinline__ void t_sincos(const D3& a, D3& s, D3& c) {
    const double sv = sin(a.v), cv = cos(a.v);
    s = {sv, {a.d[0] * cv, a.d[1] * cv, a.d[2] * cv}};
    c = {cv, {-(a.d[0] * sv), -(a.d[1] * sv), -(a.d[2] * sv)}};
}

// tracking_utils.py:91-139, expression by expression; T = double or D3 (the angle-axis entries), p plain
template <class T>
__device__ __forceinline__ void aa_rotate(const T& a0, const T& a1, const T& a2, const double (&p)[3], T (&out)[3]) {
    const T theta2 = (a0 * a0 + a1 * a1) + a2 * a2;
    if (value(theta2) > 0.0) {
        const T theta = t_sqrt(theta2);
        T s, c;
        t_sincos(theta, s, c);
        const T ti = t_recip(theta);
        const T w0 = a0 * ti, w1 = a1 * ti, w2 = a2 * ti;
        const T x0 = w1 * p[2] - w2 * p[1], x1 = w2 * p[0] - w0 * p[2], x2 = w0 * p[1] - w1 * p[0];
        const T tmp = ((w0 * p[0] + w1 * p[1]) + w2 * p[2]) * (1.0 - c);
        out[0] = (c * p[0] + x0 * s) + w0 * tmp;
        out[1] = (c * p[1] + x1 * s) + w1 * tmp;
        out[2] = (c * p[2] + x2 * s) + w2 * tmp;
    } else {  // the first-order form is the function here
        out[0] = p[0] + (a1 * p[2] - a2 * p[1]);
        out[1] = p[1] + (a2 * p[0] - a0 * p[2]);
        out[2] = p[2] + (a0 * p[1] - a1 * p[0]);
    }
}

// d (rotated point) / d p: the rotation matrix of the same branch
__device__ __forceinline__ void aa_matrix(const double (&a)[3], double (&R)[3][3]) {
    const double theta2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    double w[3] = {a[0], a[1], a[2]}, s = 1.0, c = 1.0;
    if (theta2 > 0.0) {
        const double theta = sqrt(theta2), ti = 1.0 / theta;
        s = sin(theta);
        c = cos(theta);
        for (int i = 0; i < 3; ++i) w[i] = a[i] * ti;
    }
    const double k = 1.0 - c;  // 0 in the first-order branch
    R[0][0] = c + w[0] * w[0] * k;
    R[0][1] = w[0] * w[1] * k - w[2] * s;
    R[0][2] = w[0] * w[2] * k + w[1] * s;
    R[1][0] = w[1] * w[0] * k + w[2] * s;
    R[1][1] = c + w[1] * w[1] * k;
    R[1][2] = w[1] * w[2] * k - w[0] * s;
    R[2][0] = w[2] * w[0] * k - w[1] * s;
    R[2][1] = w[2] * w[1] * k + w[0] * s;
    R[2][2] = c + w[2] * w[2] * k;
}

// the residual alone (candidate cost)
__device__ __forceinline__ void residual(const double (&cam)[6], const double* K, const double (&p)[3], const double* xy, double (&r)[2]) {
    double q[3];
    aa_rotate<double>(cam[0], cam[1], cam[2], p, q);
    const double X = q[0] + cam[3], Y = q[1] + cam[4], Z = q[2] + cam[5];
    r[0] = (K[0] * (X / Z) + K[2]) - xy[0];
    r[1] = (K[1] * (Y / Z) + K[3]) - xy[1];
}

// ---- one-time stable counting sort -----------------------------------------------------------------------------------------

// key of observation o: its camera (BY_PT = 0) or point (1); K (past every real key) when an index is out of range
template <int BY_PT>
__device__ __forceinline__ int sort_key(const int* obs_cam, const int* obs_pt, int o, int C, int P) {
    const int c = obs_cam[o], j = obs_pt[o];
    if (!in_range(c, j, C, P)) return BY_PT ? P : C;
    return BY_PT ? j : c;
}

// One pass of the LSD radix sort of the observation indices by digit (key >> shift) & 63: thread t owns the contiguous
// segment [t seg, (t + 1) seg) of src (src == nullptr: the identity) and its own column of the histogram, so the order
// inside a digit is the order of src.  LDS: RADIX * SORT_THREADS + SORT_THREADS / 64 ints (dynamic).
template <int BY_PT>
__global__ __launch_bounds__(SORT_THREADS) void ba_sort_pass_kernel(const int* __restrict__ obs_cam, const int* __restrict__ obs_pt, int C,
                                                                    int P, int M, int shift, const int* __restrict__ src,
                                                                    int* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) int sort_lds[];
    int* hist = sort_lds;                       // [RADIX][SORT_THREADS]
    int* wsum = sort_lds + RADIX * SORT_THREADS;
    const int t = threadIdx.x;
    const int seg = (M + SORT_THREADS - 1) / SORT_THREADS;
    const int lo = min(M, t * seg), hi = min(M, lo + seg);
    for (int d = 0; d < RADIX; ++d) hist[d * SORT_THREADS + t] = 0;
    for (int i = lo; i < hi; ++i) {
        const int o = src ? src[i] : i;
        const int d = (sort_key<BY_PT>(obs_cam, obs_pt, o, C, P) >> shift) & (RADIX - 1);
        hist[d * SORT_THREADS + t] += 1;
    }
    int base = 0;
    for (int d = 0; d < RADIX; ++d) {
        int total;
        const int before = wg::excl_scan<SORT_THREADS>(hist[d * SORT_THREADS + t], wsum, total);
        hist[d * SORT_THREADS + t] = base + before;
        base += total;
    }
    for (int i = lo; i < hi; ++i) {
        const int o = src ? src[i] : i;
        const int d = (sort_key<BY_PT>(obs_cam, obs_pt, o, C, P) >> shift) & (RADIX - 1);
        const int pos = hist[d * SORT_THREADS + t]++;
        if (pos < M) dst[pos] = o;
    }
}

// Group offsets of the two sorted lists: off[k] = first position whose key is >= k, k = 0 .. K (K + 1 entries; off[K] =
// number of observations in range).  blockIdx.y: 0 = cameras, 1 = points.
__global__ __launch_bounds__(LIN_THREADS) void ba_offsets_kernel(const int* __restrict__ obs_cam, const int* __restrict__ obs_pt, int C, int P,
                                                                 int M, const int* __restrict__ cam_obs, const int* __restrict__ pt_obs,
                                                                 int* __restrict__ cam_off, int* __restrict__ pt_off) {
    const int i = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (i > M) return;
    const bool by_pt = blockIdx.y != 0;
    const int K = by_pt ? P : C;
    const int* list = by_pt ? pt_obs : cam_obs;
    int* off = by_pt ? pt_off : cam_off;
    int prev = -1, cur = K + 1;
    if (i > 0) prev = by_pt ? sort_key<1>(obs_cam, obs_pt, list[i - 1], C, P) : sort_key<0>(obs_cam, obs_pt, list[i - 1], C, P);
    if (i < M) cur = by_pt ? sort_key<1>(obs_cam, obs_pt, list[i], C, P) : sort_key<0>(obs_cam, obs_pt, list[i], C, P);
    for (int k = prev + 1; k <= cur && k <= K; ++k) off[k] = i;
}

// ---- per iteration ----------------------------------------------------------------------------------------------------------

__global__ void ba_init_kernel(Ctrl* ctrl) {
    ctrl->mu = MU0;
    ctrl->nu = 2.0;
    ctrl->initial_cost = 0.0;
    ctrl->final_cost = 0.0;
    ctrl->n_acc = ctrl->n_att = ctrl->done = ctrl->accept = ctrl->status = ctrl->chol_fail = 0;
}

// r, d r / d camera, d r / d point of every observation (one thread each)
__global__ __launch_bounds__(LIN_THREADS) void ba_lin_kernel(const double* __restrict__ cams, const double* __restrict__ intr,
                                                             const double* __restrict__ points, const int* __restrict__ obs_cam,
                                                             const int* __restrict__ obs_pt, const double* __restrict__ obs_xy, int C, int P,
                                                             int M, double* __restrict__ r, double* __restrict__ Jc, double* __restrict__ Jp,
                                                             const Ctrl* ctrl) {
    if (finished(ctrl)) return;
    const int o = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (o >= M) return;
    const int c = obs_cam[o], j = obs_pt[o];
    if (!in_range(c, j, C, P)) {
        r[2 * o] = r[2 * o + 1] = 0.0;
        for (int k = 0; k < 2 * CAM; ++k) Jc[(size_t)o * 2 * CAM + k] = 0.0;
        for (int k = 0; k < 2 * PT; ++k) Jp[(size_t)o * 2 * PT + k] = 0.0;
        return;
    }
    double cam[6], p[3];
    for (int k = 0; k < 6; ++k) cam[k] = cams[c * 6 + k];
    for (int k = 0; k < 3; ++k) p[k] = points[(size_t)j * 3 + k];
    const double fx = intr[c * 4], fy = intr[c * 4 + 1], cx = intr[c * 4 + 2], cy = intr[c * 4 + 3];
    D3 q[3];
    aa_rotate<D3>(D3{cam[0], {1.0, 0.0, 0.0}}, D3{cam[1], {0.0, 1.0, 0.0}}, D3{cam[2], {0.0, 0.0, 1.0}}, p, q);
    double R[3][3];
    const double a[3] = {cam[0], cam[1], cam[2]};
    aa_matrix(a, R);
    const double X = q[0].v + cam[3], Y = q[1].v + cam[4], Z = q[2].v + cam[5];
    r[2 * o] = (fx * (X / Z) + cx) - obs_xy[2 * o];
    r[2 * o + 1] = (fy * (Y / Z) + cy) - obs_xy[2 * o + 1];
    // d r / d (X, Y, Z)
    const double iz = 1.0 / Z;
    const double A[2][3] = {{fx * iz, 0.0, -(fx * X * iz * iz)}, {0.0, fy * iz, -(fy * Y * iz * iz)}};
    double* jc = Jc + (size_t)o * 2 * CAM;
    double* jp = Jp + (size_t)o * 2 * PT;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            jc[row * CAM + k] = (A[row][0] * q[0].d[k] + A[row][1] * q[1].d[k]) + A[row][2] * q[2].d[k];
            jc[row * CAM + 3 + k] = A[row][k];
            jp[row * PT + k] = (A[row][0] * R[0][k] + A[row][1] * R[1][k]) + A[row][2] * R[2][k];
        }
    }
}

// U_c (upper triangle accumulated, written symmetric), g_c and the cost of camera blockIdx.x: thread t sums the
// observations t, t + CAM_THREADS, .. of the camera's list, then a tree over the threads.
__global__ __launch_bounds__(CAM_THREADS) void ba_cam_blocks_kernel(const double* __restrict__ r, const double* __restrict__ Jc,
                                                                    const int* __restrict__ cam_obs, const int* __restrict__ cam_off,
                                                                    const int* __restrict__ cam_fixed, double* __restrict__ U,
                                                                    double* __restrict__ g_c, double* __restrict__ cost_cam, const Ctrl* ctrl) {
    constexpr int Q = 21 + CAM + 1;
    __shared__ double red[Q * CAM_THREADS];
    if (finished(ctrl)) return;
    const int c = blockIdx.x, t = threadIdx.x;
    const int lo = cam_off[c], hi = cam_off[c + 1];
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int i = lo + t; i < hi; i += CAM_THREADS) {
        const int o = cam_obs[i];
        const double r0 = r[2 * o], r1 = r[2 * o + 1];
        double j[2 * CAM];
#pragma unroll
        for (int k = 0; k < 2 * CAM; ++k) j[k] = Jc[(size_t)o * 2 * CAM + k];
        int q = 0;
#pragma unroll
        for (int a = 0; a < CAM; ++a)
#pragma unroll
            for (int b = a; b < CAM; ++b) acc[q++] += j[a] * j[b] + j[CAM + a] * j[CAM + b];
#pragma unroll
        for (int a = 0; a < CAM; ++a) acc[21 + a] += j[a] * r0 + j[CAM + a] * r1;
        acc[Q - 1] += 0.5 * (r0 * r0 + r1 * r1);
    }
    wg::tree_sum<CAM_THREADS, Q>(acc, red);
    const bool fixed = cam_fixed && cam_fixed[c] != 0;
    if (t < CAM * CAM) {
        const int a = t / CAM, b = t % CAM, lo_ = a < b ? a : b, hi_ = a < b ? b : a;
        // index of (lo_, hi_) in the row-major upper triangle
        const int q = lo_ * CAM - lo_ * (lo_ - 1) / 2 + (hi_ - lo_);
        U[c * CAM * CAM + t] = fixed ? 0.0 : red[q * CAM_THREADS];  // tree_sum leaves the totals in red[q][0]
    }
    if (t < CAM) g_c[c * CAM + t] = fixed ? 0.0 : red[(21 + t) * CAM_THREADS];
    if (t == 0) cost_cam[c] = acc[Q - 1];
}

// V_j and g_p of point j (one thread each), the observations of the point in input order
__global__ __launch_bounds__(LIN_THREADS) void ba_pt_blocks_kernel(const double* __restrict__ r, const double* __restrict__ Jp,
                                                                   const int* __restrict__ pt_obs, const int* __restrict__ pt_off,
                                                                   const int* __restrict__ pt_fixed, int P, double* __restrict__ V,
                                                                   double* __restrict__ g_p, const Ctrl* ctrl) {
    if (finished(ctrl)) return;
    const int j = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (j >= P) return;
    double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    if (!(pt_fixed && pt_fixed[j] != 0)) {
        for (int i = pt_off[j]; i < pt_off[j + 1]; ++i) {
            const int o = pt_obs[i];
            const double r0 = r[2 * o], r1 = r[2 * o + 1];
            double q[2 * PT];
#pragma unroll
            for (int k = 0; k < 2 * PT; ++k) q[k] = Jp[(size_t)o * 2 * PT + k];
            v[0] += q[0] * q[0] + q[3] * q[3];
            v[1] += q[0] * q[1] + q[3] * q[4];
            v[2] += q[0] * q[2] + q[3] * q[5];
            v[3] += q[1] * q[1] + q[4] * q[4];
            v[4] += q[1] * q[2] + q[4] * q[5];
            v[5] += q[2] * q[2] + q[5] * q[5];
#pragma unroll
            for (int k = 0; k < PT; ++k) g[k] += q[k] * r0 + q[PT + k] * r1;
        }
    }
    double* out = V + (size_t)j * 9;
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
    out[3] = v[1]; out[4] = v[3]; out[5] = v[4];
    out[6] = v[2]; out[7] = v[4]; out[8] = v[5];
    for (int k = 0; k < PT; ++k) g_p[(size_t)j * 3 + k] = g[k];
}

// inverse of the symmetric 3x3 V + clamp(diag V) / mu in closed form (adjugate / determinant)
__device__ __forceinline__ void damped_inverse(const double* V, double mu, double (&inv)[9]) {
    const double a = V[0] + clamp_diag(V[0]) / mu, b = V[1], c = V[2], d = V[4] + clamp_diag(V[4]) / mu, e = V[5],
                 f = V[8] + clamp_diag(V[8]) / mu;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = (a * c00 + b * c01) + c * c02;
    const double id = 1.0 / det;
    inv[0] = c00 * id;
    inv[1] = inv[3] = c01 * id;
    inv[2] = inv[6] = c02 * id;
    inv[4] = (a * f - c * c) * id;
    inv[5] = inv[7] = (b * c - a * e) * id;
    inv[8] = (a * d - b * b) * id;
}

__device__ __forceinline__ bool cam_active(int c, const int* cam_fixed, const int* cam_off) {
    return !(cam_fixed && cam_fixed[c] != 0) && cam_off[c + 1] > cam_off[c];
}
__device__ __forceinline__ bool pt_active(int j, const int* pt_fixed, const int* pt_off) {
    return !(pt_fixed && pt_fixed[j] != 0) && pt_off[j + 1] > pt_off[j];
}

// Schur partial of the points [blockIdx.x chunk, (blockIdx.x + 1) chunk): partial [n][n + 1], n = 6 C, accumulates
// W_j Vinv_j W_j^T (columns 0 .. n - 1) and W_j Vinv_j g_pj (column n), point after point in index order.  W_cj is the sum
// of Jc_o^T Jp_o over the observations of point j by camera c in input order.  A thread owns different entries from one
// point to the next: the barrier between two points orders those global read-modify-writes inside the workgroup.
__global__ __launch_bounds__(SCHUR_THREADS) void ba_schur_partial_kernel(const double* __restrict__ V, const double* __restrict__ g_p,
                                                                         const double* __restrict__ Jc, const double* __restrict__ Jp,
                                                                         const int* __restrict__ obs_cam, const int* __restrict__ pt_obs,
                                                                         const int* __restrict__ pt_off, const int* __restrict__ cam_fixed,
                                                                         const int* __restrict__ pt_fixed, int C, int P, int chunk,
                                                                         double mu_host, double* partial, const Ctrl* ctrl) {
    __shared__ int slot[BA_MAX_CAMERAS], cam_of[BA_MAX_CAMERAS], n_slots;
    __shared__ double W[BA_MAX_CAMERAS][CAM * PT], WV[BA_MAX_CAMERAS][CAM * PT], vinv[9], gpj[3];
    if (finished(ctrl)) return;
    const double mu = ctrl ? ctrl->mu : mu_host;
    const int t = threadIdx.x, n = CAM * C, stride = n + 1;
    double* mine = partial + (size_t)blockIdx.x * n * stride;
    for (int e = t; e < n * stride; e += SCHUR_THREADS) mine[e] = 0.0;
    const int j0 = blockIdx.x * chunk, j1 = min(P, j0 + chunk);
    for (int j = j0; j < j1; ++j) {
        if (!pt_active(j, pt_fixed, pt_off)) continue;  // uniform over the workgroup
        const int lo = pt_off[j], hi = pt_off[j + 1];
        __syncthreads();  // the previous point's LDS reads and partial updates are done
        if (t < C) slot[t] = -1;
        __syncthreads();
        if (t == 0) {
            int ns = 0;
            for (int i = lo; i < hi; ++i) {
                const int c = obs_cam[pt_obs[i]];
                if (slot[c] < 0 && !(cam_fixed && cam_fixed[c] != 0)) {
                    slot[c] = ns;
                    cam_of[ns++] = c;
                }
            }
            n_slots = ns;
            double inv[9];
            damped_inverse(V + (size_t)j * 9, mu, inv);
            for (int k = 0; k < 9; ++k) vinv[k] = inv[k];
            for (int k = 0; k < 3; ++k) gpj[k] = g_p[(size_t)j * 3 + k];
        }
        __syncthreads();
        const int ns = n_slots;
        for (int item = t; item < ns * CAM * PT; item += SCHUR_THREADS) {
            const int s = item / (CAM * PT), e = item % (CAM * PT), a = e / PT, m = e % PT, c = cam_of[s];
            double w = 0.0;
            for (int i = lo; i < hi; ++i) {
                const int o = pt_obs[i];
                if (obs_cam[o] != c) continue;
                const double* jc = Jc + (size_t)o * 2 * CAM;
                const double* jp = Jp + (size_t)o * 2 * PT;
                w += jc[a] * jp[m] + jc[CAM + a] * jp[PT + m];
            }
            W[s][e] = w;
        }
        __syncthreads();
        for (int item = t; item < ns * CAM * PT; item += SCHUR_THREADS) {
            const int s = item / (CAM * PT), e = item % (CAM * PT), a = e / PT, m = e % PT;
            WV[s][e] = (W[s][a * PT] * vinv[m] + W[s][a * PT + 1] * vinv[3 + m]) + W[s][a * PT + 2] * vinv[6 + m];
        }
        __syncthreads();
        const int rows = ns * CAM, cols = rows + 1;
        for (int item = t; item < rows * cols; item += SCHUR_THREADS) {
            const int ra = item / cols, rb = item % cols;
            const int sa = ra / CAM, a = ra % CAM;
            const int row = cam_of[sa] * CAM + a;
            const double* wv = &WV[sa][a * PT];
            if (rb < rows) {
                const int sb = rb / CAM, b = rb % CAM;
                const double* w = &W[sb][b * PT];
                mine[(size_t)row * stride + cam_of[sb] * CAM + b] += (wv[0] * w[0] + wv[1] * w[1]) + wv[2] * w[2];
            } else {
                mine[(size_t)row * stride + n] += (wv[0] * gpj[0] + wv[1] * gpj[1]) + wv[2] * gpj[2];
            }
        }
    }
}

// S = U + D^2 / mu - sum over the chunks, rhs = -g_c + sum over the chunks, chunk after chunk; the rows and columns of a
// fixed or unobserved camera are those of the identity with a zero right-hand side.
__global__ __launch_bounds__(LIN_THREADS) void ba_schur_reduce_kernel(const double* __restrict__ U, const double* __restrict__ g_c,
                                                                      const double* __restrict__ partial, int n_chunks,
                                                                      const int* __restrict__ cam_off, const int* __restrict__ cam_fixed, int C,
                                                                      double mu_host, double* __restrict__ S, double* __restrict__ rhs,
                                                                      const Ctrl* ctrl) {
    if (finished(ctrl)) return;
    const double mu = ctrl ? ctrl->mu : mu_host;
    const int n = CAM * C, stride = n + 1;
    const int e = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (e >= n * stride) return;
    const int a = e / stride, b = e % stride, ca = a / CAM;
    const bool act_a = cam_active(ca, cam_fixed, cam_off);
    if (b == n) {
        double sum = 0.0;
        if (act_a)
            for (int ch = 0; ch < n_chunks; ++ch) sum += partial[(size_t)ch * n * stride + e];
        rhs[a] = act_a ? sum - g_c[a] : 0.0;
        return;
    }
    const int cb = b / CAM;
    if (!act_a || !cam_active(cb, cam_fixed, cam_off)) {
        S[a * n + b] = a == b ? 1.0 : 0.0;
        return;
    }
    double val = 0.0;
    if (ca == cb) {
        val = U[ca * CAM * CAM + (a % CAM) * CAM + (b % CAM)];
        if (a == b) val += clamp_diag(val) / mu;
    }
    double sum = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) sum += partial[(size_t)ch * n * stride + e];
    S[a * n + b] = val - sum;
}

// Cholesky of S (packed lower triangle in LDS, right-looking) and the camera step: one workgroup.
// LDS: n (n + 1) / 2 + n doubles (dynamic).
__global__ __launch_bounds__(CHOL_THREADS) void ba_cholesky_kernel(const double* __restrict__ S, const double* __restrict__ rhs, int n,
                                                                   double* __restrict__ delta_c, Ctrl* ctrl, int* fail_out) {
    extern __shared__ __attribute__((aligned(16))) double chol_lds[];
    __shared__ int bad;
    if (finished(ctrl)) return;
    double* L = chol_lds;
    double* x = chol_lds + n * (n + 1) / 2;
    const int t = threadIdx.x;
    auto at = [](int i, int j) { return i * (i + 1) / 2 + j; };
    for (int i = t / 16; i < n; i += CHOL_THREADS / 16)
        for (int j = t % 16; j <= i; j += 16) L[at(i, j)] = S[i * n + j];
    for (int i = t; i < n; i += CHOL_THREADS) x[i] = rhs[i];
    if (t == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (t == 0) {
            double d = L[at(k, k)];
            if (!(d > 0.0) || !(d <= DIAG_MAX * DIAG_MAX)) {
                bad = 1;
                d = 1.0;
            }
            L[at(k, k)] = sqrt(d);
        }
        __syncthreads();
        const double lkk = L[at(k, k)];
        for (int i = k + 1 + t; i < n; i += CHOL_THREADS) L[at(i, k)] = L[at(i, k)] / lkk;
        __syncthreads();
        for (int i = k + 1 + t / 16; i < n; i += CHOL_THREADS / 16) {
            const double lik = L[at(i, k)];
            for (int j = k + 1 + t % 16; j <= i; j += 16) L[at(i, j)] -= lik * L[at(j, k)];
        }
        __syncthreads();
    }
    // L y = rhs
    for (int k = 0; k < n; ++k) {
        if (t == 0) x[k] = x[k] / L[at(k, k)];
        __syncthreads();
        const double yk = x[k];
        for (int i = k + 1 + t; i < n; i += CHOL_THREADS) x[i] -= L[at(i, k)] * yk;
        __syncthreads();
    }
    // L^T delta = y
    for (int k = n - 1; k >= 0; --k) {
        if (t == 0) x[k] = x[k] / L[at(k, k)];
        __syncthreads();
        const double xk = x[k];
        for (int i = t; i < k; i += CHOL_THREADS) x[i] -= L[at(k, i)] * xk;
        __syncthreads();
    }
    const bool failed = bad != 0;
    for (int i = t; i < n; i += CHOL_THREADS) delta_c[i] = failed ? 0.0 : x[i];
    if (t == 0) {
        if (ctrl) ctrl->chol_fail = failed;
        if (fail_out) *fail_out = failed;
    }
}

// delta_p of point j = -Vinv_j (g_pj + sum over its observations of Jp_o^T (Jc_o delta_c)), input order (one thread each)
__global__ __launch_bounds__(LIN_THREADS) void ba_backsub_kernel(const double* __restrict__ V, const double* __restrict__ g_p,
                                                                 const double* __restrict__ Jc, const double* __restrict__ Jp,
                                                                 const int* __restrict__ obs_cam, const int* __restrict__ pt_obs,
                                                                 const int* __restrict__ pt_off, const int* __restrict__ pt_fixed, int P,
                                                                 double mu_host, const double* __restrict__ delta_c, double* __restrict__ delta_p,
                                                                 const Ctrl* ctrl, const int* fail) {
    if (finished(ctrl)) return;
    const double mu = ctrl ? ctrl->mu : mu_host;
    const int j = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (j >= P) return;
    double d[3] = {0.0, 0.0, 0.0};
    if (pt_active(j, pt_fixed, pt_off) && !*fail) {
        double s[3];
        for (int k = 0; k < 3; ++k) s[k] = g_p[(size_t)j * 3 + k];
        for (int i = pt_off[j]; i < pt_off[j + 1]; ++i) {
            const int o = pt_obs[i];
            const double* jc = Jc + (size_t)o * 2 * CAM;
            const double* jp = Jp + (size_t)o * 2 * PT;
            const double* dc = delta_c + obs_cam[o] * CAM;
            double u0 = 0.0, u1 = 0.0;
#pragma unroll
            for (int k = 0; k < CAM; ++k) {
                u0 += jc[k] * dc[k];
                u1 += jc[CAM + k] * dc[k];
            }
#pragma unroll
            for (int k = 0; k < PT; ++k) s[k] += jp[k] * u0 + jp[PT + k] * u1;
        }
        double inv[9];
        damped_inverse(V + (size_t)j * 9, mu, inv);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = -((inv[k * 3] * s[0] + inv[k * 3 + 1] * s[1]) + inv[k * 3 + 2] * s[2]);
    }
    for (int k = 0; k < 3; ++k) delta_p[(size_t)j * 3 + k] = d[k];
}

// model decrease = -sum over the observations of (r . J delta + 1/2 |J delta|^2): one workgroup, thread t sums the entries
// t, t + MODEL_THREADS, .. of the point-sorted list (observations in range only), then a tree.
__global__ __launch_bounds__(MODEL_THREADS) void ba_model_kernel(const double* __restrict__ r, const double* __restrict__ Jc,
                                                                 const double* __restrict__ Jp, const int* __restrict__ obs_cam,
                                                                 const int* __restrict__ obs_pt, const int* __restrict__ pt_obs,
                                                                 const int* __restrict__ pt_off, int P, const double* __restrict__ delta_c,
                                                                 const double* __restrict__ delta_p, double* __restrict__ model_decrease,
                                                                 const Ctrl* ctrl) {
    __shared__ double red[MODEL_THREADS];
    if (finished(ctrl)) return;
    double acc[1] = {0.0};
    const int n_obs = pt_off[P];
    for (int i = threadIdx.x; i < n_obs; i += MODEL_THREADS) {
        const int o = pt_obs[i], c = obs_cam[o], j = obs_pt[o];
        const double* jc = Jc + (size_t)o * 2 * CAM;
        const double* jp = Jp + (size_t)o * 2 * PT;
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < CAM; ++k) {
            u0 += jc[k] * delta_c[c * CAM + k];
            u1 += jc[CAM + k] * delta_c[c * CAM + k];
        }
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            u0 += jp[k] * delta_p[(size_t)j * 3 + k];
            u1 += jp[PT + k] * delta_p[(size_t)j * 3 + k];
        }
        acc[0] += (r[2 * o] * u0 + r[2 * o + 1] * u1) + 0.5 * (u0 * u0 + u1 * u1);
    }
    wg::tree_sum<MODEL_THREADS, 1>(acc, red);
    if (threadIdx.x == 0) *model_decrease = -acc[0];
}

// cost of camera blockIdx.x at cams + delta_c, points + delta_p: the summation order of ba_cam_blocks_kernel
__global__ __launch_bounds__(CAM_THREADS) void ba_candidate_kernel(const double* __restrict__ cams, const double* __restrict__ intr,
                                                                   const double* __restrict__ points, const int* __restrict__ obs_pt,
                                                                   const double* __restrict__ obs_xy, const int* __restrict__ cam_obs,
                                                                   const int* __restrict__ cam_off, const double* __restrict__ delta_c,
                                                                   const double* __restrict__ delta_p, double* __restrict__ cand_cam,
                                                                   const Ctrl* ctrl) {
    __shared__ double red[CAM_THREADS];
    if (finished(ctrl)) return;
    const int c = blockIdx.x, t = threadIdx.x;
    double cam[6];
    for (int k = 0; k < 6; ++k) cam[k] = cams[c * 6 + k] + delta_c[c * 6 + k];
    double acc[1] = {0.0};
    for (int i = cam_off[c] + t; i < cam_off[c + 1]; i += CAM_THREADS) {
        const int o = cam_obs[i], j = obs_pt[o];
        double p[3], res[2];
        for (int k = 0; k < 3; ++k) p[k] = points[(size_t)j * 3 + k] + delta_p[(size_t)j * 3 + k];
        residual(cam, intr + c * 4, p, obs_xy + 2 * (size_t)o, res);
        acc[0] += 0.5 * (res[0] * res[0] + res[1] * res[1]);
    }
    wg::tree_sum<CAM_THREADS, 1>(acc, red);
    if (t == 0) cand_cam[c] = acc[0];
}

// rho, accept / reject, the mu update, the trace row and the summary: one thread
__global__ void ba_decide_kernel(Ctrl* ctrl, const double* __restrict__ cost_cam, const double* __restrict__ cand_cam,
                                 const double* __restrict__ model_decrease, const int* __restrict__ pt_off, int C, int P, int M, int it,
                                 int num_success, double* __restrict__ trace, double* __restrict__ summary) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double* row = trace + (size_t)it * BA_TRACE_COLUMNS;
    if (ctrl->done) {
        for (int k = 0; k < BA_TRACE_COLUMNS - 1; ++k) row[k] = 0.0;
        row[BA_TRACE_COLUMNS - 1] = -1.0;
        ctrl->accept = 0;
        return;
    }
    double cost = 0.0, cand = 0.0;
    for (int c = 0; c < C; ++c) cost += cost_cam[c];
    for (int c = 0; c < C; ++c) cand += cand_cam[c];
    if (it == 0) {
        ctrl->initial_cost = ctrl->final_cost = cost;
        if (!isfinite(cost)) {
            ctrl->status = BA_STATUS_NONFINITE_START;
            ctrl->done = 1;
        }
    }
    int accepted = 0;
    if (ctrl->done) {
        for (int k = 0; k < BA_TRACE_COLUMNS - 1; ++k) row[k] = 0.0;
        row[0] = cost;
        row[BA_TRACE_COLUMNS - 1] = -1.0;
    } else {
        const double md = *model_decrease, mu = ctrl->mu;
        const double rho = (cost - cand) / md;
        accepted = !ctrl->chol_fail && isfinite(cand) && md > 0.0 && rho > MIN_RHO;
        row[0] = cost;
        row[1] = cand;
        row[2] = md;
        row[3] = rho;
        row[4] = mu;
        row[5] = accepted ? 1.0 : 0.0;
        ctrl->n_att += 1;
        if (accepted) {
            const double u = 2.0 * rho - 1.0;
            ctrl->mu = fmin(mu / fmax(1.0 / 3.0, 1.0 - u * u * u), MU_MAX);
            ctrl->nu = 2.0;
            ctrl->n_acc += 1;
            ctrl->final_cost = cand;
            if (ctrl->n_acc >= num_success) ctrl->done = 1;
        } else {
            ctrl->mu = mu / ctrl->nu;
            ctrl->nu = 2.0 * ctrl->nu;
        }
    }
    ctrl->accept = accepted;
    summary[0] = ctrl->initial_cost;
    summary[1] = ctrl->final_cost;
    summary[2] = (double)ctrl->n_acc;
    summary[3] = (double)ctrl->n_att;
    summary[4] = (double)(M - pt_off[P]);
    summary[5] = (double)ctrl->status;
}

// cams += delta_c, points += delta_p when the step was accepted; a fixed or unobserved variable is not written
__global__ __launch_bounds__(LIN_THREADS) void ba_apply_kernel(const Ctrl* ctrl, const double* __restrict__ delta_c,
                                                               const double* __restrict__ delta_p, const int* __restrict__ cam_off,
                                                               const int* __restrict__ pt_off, const int* __restrict__ cam_fixed,
                                                               const int* __restrict__ pt_fixed, int C, int P, double* __restrict__ cams,
                                                               double* __restrict__ points) {
    if (!ctrl->accept) return;
    const int e = blockIdx.x * LIN_THREADS + threadIdx.x;
    if (e < CAM * C) {
        if (cam_active(e / CAM, cam_fixed, cam_off)) cams[e] += delta_c[e];
    } else if (e < CAM * C + PT * P) {
        const int k = e - CAM * C;
        if (pt_active(k / PT, pt_fixed, pt_off)) points[k] += delta_p[k];
    }
}

}  // namespace bak

using namespace bak;
using namespace capi;

namespace {

int chunk_points(int P) { return std::max(MIN_CHUNK_POINTS, ceil_div(P, MAX_CHUNKS)); }
int chunk_count(int P) { return ceil_div(P, chunk_points(P)); }

struct Workspace {
    Ctrl* ctrl;
    int *cam_obs, *pt_obs, *tmp, *cam_off, *pt_off, *fail;
    double *r, *Jc, *Jp, *U, *V, *g_c, *g_p, *cost_cam, *cand_cam, *md, *partial, *S, *rhs, *dc, *dp;
    size_t bytes;
};

Workspace carve(void* base, int C, int P, int M) {
    Bump b(base);
    Workspace w;
    const size_t n = (size_t)CAM * C;
    w.ctrl = b.take<Ctrl>(sizeof(Ctrl));
    w.fail = b.take<int>(sizeof(int));
    w.cam_obs = b.take<int>(sizeof(int) * M);
    w.pt_obs = b.take<int>(sizeof(int) * M);
    w.tmp = b.take<int>(sizeof(int) * M);
    w.cam_off = b.take<int>(sizeof(int) * (C + 1));
    w.pt_off = b.take<int>(sizeof(int) * ((size_t)P + 1));
    w.r = b.take<double>(sizeof(double) * 2 * M);
    w.Jc = b.take<double>(sizeof(double) * 2 * CAM * M);
    w.Jp = b.take<double>(sizeof(double) * 2 * PT * M);
    w.U = b.take<double>(sizeof(double) * CAM * n);
    w.V = b.take<double>(sizeof(double) * 9 * P);
    w.g_c = b.take<double>(sizeof(double) * n);
    w.g_p = b.take<double>(sizeof(double) * 3 * P);
    w.cost_cam = b.take<double>(sizeof(double) * C);
    w.cand_cam = b.take<double>(sizeof(double) * C);
    w.md = b.take<double>(sizeof(double));
    w.partial = b.take<double>(sizeof(double) * chunk_count(P) * n * (n + 1));
    w.S = b.take<double>(sizeof(double) * n * n);
    w.rhs = b.take<double>(sizeof(double) * n);
    w.dc = b.take<double>(sizeof(double) * n);
    w.dp = b.take<double>(sizeof(double) * 3 * P);
    w.bytes = b.off;
    return w;
}

int check_sizes(const char* who, int C, int P, int M) {
    if (C < 1 || C > BA_MAX_CAMERAS || P < 1 || P > BA_MAX_POINTS || M < 1 || M > BA_MAX_OBSERVATIONS)
        return fail(-1, "%s: C in [1, %d], P in [1, %d] and M in [1, %d] expected (got %d, %d, %d)", who, BA_MAX_CAMERAS, BA_MAX_POINTS,
                    BA_MAX_OBSERVATIONS, C, P, M);
    return 0;
}

int radix_passes(int K) {  // keys 0 .. K inclusive
    int passes = 1;
    while ((K >> (RADIX_BITS * passes)) != 0) ++passes;
    return passes;
}

template <int BY_PT>
bool sort_list(const int32_t* obs_cam, const int32_t* obs_pt, int C, int P, int M, int* dst, int* tmp, hipStream_t s) {
    const size_t lds = sizeof(int) * (RADIX * SORT_THREADS + SORT_THREADS / 64);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ba_sort_pass_kernel<BY_PT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
        return false;
    const int passes = radix_passes(BY_PT ? P : C);
    const int* src = nullptr;
    for (int k = 0; k < passes; ++k) {
        int* out = (passes - 1 - k) % 2 == 0 ? dst : tmp;
        hipLaunchKernelGGL(ba_sort_pass_kernel<BY_PT>, dim3(1), dim3(SORT_THREADS), lds, s, obs_cam, obs_pt, C, P, M, RADIX_BITS * k, src, out);
        src = out;
    }
    return true;
}

// the one-time sort: w.cam_obs / w.pt_obs and their group offsets
bool enqueue_sort(const Workspace& w, const int32_t* obs_cam, const int32_t* obs_pt, int C, int P, int M, hipStream_t s) {
    if (!sort_list<0>(obs_cam, obs_pt, C, P, M, w.cam_obs, w.tmp, s)) return false;
    if (!sort_list<1>(obs_cam, obs_pt, C, P, M, w.pt_obs, w.tmp, s)) return false;
    hipLaunchKernelGGL(ba_offsets_kernel, dim3(ceil_div(M + 1, LIN_THREADS), 2), dim3(LIN_THREADS), 0, s, obs_cam, obs_pt, C, P, M,
                       w.cam_obs, w.pt_obs, w.cam_off, w.pt_off);
    return true;
}

void enqueue_linearize(const double* cams, const double* intr, const double* points, const int32_t* obs_cam, const int32_t* obs_pt,
                       const double* obs_xy, int C, int P, int M, double* r, double* Jc, double* Jp, const Ctrl* ctrl, hipStream_t s) {
    hipLaunchKernelGGL(ba_lin_kernel, dim3(ceil_div(M, LIN_THREADS)), dim3(LIN_THREADS), 0, s, cams, intr, points, obs_cam, obs_pt,
                       obs_xy, C, P, M, r, Jc, Jp, ctrl);
}

void enqueue_blocks(const Workspace& w, const double* r, const double* Jc, const double* Jp, const int32_t* cam_fixed, const int32_t* pt_fixed,
                    int C, int P, double* U, double* V, double* g_c, double* g_p, double* cost_cam, const Ctrl* ctrl, hipStream_t s) {
    hipLaunchKernelGGL(ba_cam_blocks_kernel, dim3(C), dim3(CAM_THREADS), 0, s, r, Jc, w.cam_obs, w.cam_off, cam_fixed, U, g_c, cost_cam, ctrl);
    hipLaunchKernelGGL(ba_pt_blocks_kernel, dim3(ceil_div(P, LIN_THREADS)), dim3(LIN_THREADS), 0, s, r, Jp, w.pt_obs, w.pt_off, pt_fixed,
                       P, V, g_p, ctrl);
}

bool enqueue_step(const Workspace& w, const double* U, const double* V, const double* g_c, const double* g_p, const double* r, const double* Jc,
                  const double* Jp, const int32_t* obs_cam, const int32_t* obs_pt, const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P,
                  int M, double mu, double* dc, double* dp, double* md, Ctrl* ctrl, hipStream_t s) {
    const int n = CAM * C, chunks = chunk_count(P);
    const size_t lds = sizeof(double) * ((size_t)n * (n + 1) / 2 + n);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ba_cholesky_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(ba_schur_partial_kernel, dim3(chunks), dim3(SCHUR_THREADS), 0, s, V, g_p, Jc, Jp, obs_cam, w.pt_obs, w.pt_off, cam_fixed,
                       pt_fixed, C, P, chunk_points(P), mu, w.partial, ctrl);
    hipLaunchKernelGGL(ba_schur_reduce_kernel, dim3(ceil_div(n * (n + 1), LIN_THREADS)), dim3(LIN_THREADS), 0, s, U, g_c, w.partial, chunks,
                       w.cam_off, cam_fixed, C, mu, w.S, w.rhs, ctrl);
    hipLaunchKernelGGL(ba_cholesky_kernel, dim3(1), dim3(CHOL_THREADS), lds, s, w.S, w.rhs, n, dc, ctrl, w.fail);
    hipLaunchKernelGGL(ba_backsub_kernel, dim3(ceil_div(P, LIN_THREADS)), dim3(LIN_THREADS), 0, s, V, g_p, Jc, Jp, obs_cam, w.pt_obs,
                       w.pt_off, pt_fixed, P, mu, dc, dp, ctrl, w.fail);
    hipLaunchKernelGGL(ba_model_kernel, dim3(1), dim3(MODEL_THREADS), 0, s, r, Jc, Jp, obs_cam, obs_pt, w.pt_obs, w.pt_off, P, dc, dp, md, ctrl);
    return true;
}

}  // namespace

extern "C" {

size_t ba_workspace_bytes(int C, int P, int M) {
    if (check_sizes("ba_workspace_bytes", C, P, M) != 0) return 0;
    return carve(nullptr, C, P, M).bytes;
}

int ba_linearize(const double* cams, const double* intr, const double* points, const int32_t* obs_cam, const int32_t* obs_pt,
                 const double* obs_xy, int C, int P, int M, double* r, double* Jc, double* Jp, map_stream_t stream) {
    if (!cams || !intr || !points || !obs_cam || !obs_pt || !obs_xy || !r || !Jc || !Jp) return fail(-1, "ba_linearize: null argument");
    if (int rc = check_sizes("ba_linearize", C, P, M)) return rc;
    enqueue_linearize(cams, intr, points, obs_cam, obs_pt, obs_xy, C, P, M, r, Jc, Jp, nullptr, reinterpret_cast<hipStream_t>(stream));
    return check_launch(-3, "ba_linearize");
}

int ba_normal_blocks(const double* r, const double* Jc, const double* Jp, const int32_t* obs_cam, const int32_t* obs_pt,
                     const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P, int M, double* U, double* V, double* g_c, double* g_p,
                     double* cost_cam, void* workspace, size_t workspace_bytes, map_stream_t stream) {
    if (!r || !Jc || !Jp || !obs_cam || !obs_pt || !U || !V || !g_c || !g_p || !cost_cam) return fail(-1, "ba_normal_blocks: null argument");
    if (int rc = check_sizes("ba_normal_blocks", C, P, M)) return rc;
    if (int rc = check_workspace("ba_normal_blocks", workspace, workspace_bytes, carve(nullptr, C, P, M).bytes)) return rc;
    const Workspace w = carve(workspace, C, P, M);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!enqueue_sort(w, obs_cam, obs_pt, C, P, M, s)) return check_launch(-3, "ba_normal_blocks");
    enqueue_blocks(w, r, Jc, Jp, cam_fixed, pt_fixed, C, P, U, V, g_c, g_p, cost_cam, nullptr, s);
    return check_launch(-3, "ba_normal_blocks");
}

int ba_step(const double* U, const double* V, const double* g_c, const double* g_p, const double* r, const double* Jc, const double* Jp,
            const int32_t* obs_cam, const int32_t* obs_pt, const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P, int M, double mu,
            double* delta_c, double* delta_p, double* model_decrease, void* workspace, size_t workspace_bytes, map_stream_t stream) {
    if (!U || !V || !g_c || !g_p || !r || !Jc || !Jp || !obs_cam || !obs_pt || !delta_c || !delta_p || !model_decrease)
        return fail(-1, "ba_step: null argument");
    if (int rc = check_sizes("ba_step", C, P, M)) return rc;
    if (!(mu > 0.0) || !(mu <= MU_MAX)) return fail(-1, "ba_step: mu in (0, 1e16] expected");
    if (int rc = check_workspace("ba_step", workspace, workspace_bytes, carve(nullptr, C, P, M).bytes)) return rc;
    const Workspace w = carve(workspace, C, P, M);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!enqueue_sort(w, obs_cam, obs_pt, C, P, M, s)) return check_launch(-3, "ba_step");
    enqueue_step(w, U, V, g_c, g_p, r, Jc, Jp, obs_cam, obs_pt, cam_fixed, pt_fixed, C, P, M, mu, delta_c, delta_p, model_decrease, nullptr, s);
    return check_launch(-3, "ba_step");
}

int ba_solve(double* cams, const double* intr, double* points, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
             const int32_t* cam_fixed, const int32_t* pt_fixed, int C, int P, int M, int num_iterations, int num_success_iterations,
             double* trace, double* summary, void* workspace, size_t workspace_bytes, map_stream_t stream) {
    if (!cams || !intr || !points || !obs_cam || !obs_pt || !obs_xy || !trace || !summary) return fail(-1, "ba_solve: null argument");
    if (int rc = check_sizes("ba_solve", C, P, M)) return rc;
    if (num_iterations < 1 || num_iterations > BA_MAX_ITERATIONS || num_success_iterations < 1)
        return fail(-1, "ba_solve: num_iterations in [1, %d] and num_success_iterations >= 1 expected (got %d, %d)", BA_MAX_ITERATIONS,
                    num_iterations, num_success_iterations);
    if (int rc = check_workspace("ba_solve", workspace, workspace_bytes, carve(nullptr, C, P, M).bytes)) return rc;
    const Workspace w = carve(workspace, C, P, M);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(1), 0, s, w.ctrl);
    if (!enqueue_sort(w, obs_cam, obs_pt, C, P, M, s)) return check_launch(-3, "ba_solve");
    const int apply_blocks = ceil_div(CAM * C + PT * P, LIN_THREADS);
    for (int it = 0; it < num_iterations; ++it) {
        enqueue_linearize(cams, intr, points, obs_cam, obs_pt, obs_xy, C, P, M, w.r, w.Jc, w.Jp, w.ctrl, s);
        enqueue_blocks(w, w.r, w.Jc, w.Jp, cam_fixed, pt_fixed, C, P, w.U, w.V, w.g_c, w.g_p, w.cost_cam, w.ctrl, s);
        if (!enqueue_step(w, w.U, w.V, w.g_c, w.g_p, w.r, w.Jc, w.Jp, obs_cam, obs_pt, cam_fixed, pt_fixed, C, P, M, 0.0, w.dc, w.dp, w.md, w.ctrl, s))
            return check_launch(-3, "ba_solve");
        hipLaunchKernelGGL(ba_candidate_kernel, dim3(C), dim3(CAM_THREADS), 0, s, cams, intr, points, obs_pt, obs_xy, w.cam_obs, w.cam_off, w.dc,
                           w.dp, w.cand_cam, w.ctrl);
        hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(1), 0, s, w.ctrl, w.cost_cam, w.cand_cam, w.md, w.pt_off, C, P, M, it,
                           num_success_iterations, trace, summary);
        hipLaunchKernelGGL(ba_apply_kernel, dim3(apply_blocks), dim3(LIN_THREADS), 0, s, w.ctrl, w.dc, w.dp, w.cam_off, w.pt_off, cam_fixed, pt_fixed,
                           C, P, cams, points);
    }
    return check_launch(-3, "ba_solve");
}

}  // extern "C"
