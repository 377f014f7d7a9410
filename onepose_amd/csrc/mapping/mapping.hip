// Object database builder (C ABI: include/mapping/mapping.h; reference: run.py:80-163, src/sfm/triangulation.py,
// src/sfm/postprocess/filter_tkl.py, filter_points.py, feature_process.py).
//
// fp64 geometry on fp32 keypoints.  Small latency-bound work, no MFMA:
//   map_verify_kernel     one workgroup per image pair: epipolar test of every match against the known relative pose,
//                         ordered compaction of the survivors (wg::excl_scan)
//   map_tri_kernel<64>    one wave per track of up to 64 observations; <256>: one workgroup per longer track.  The track's
//                         observations (camera, centre, ray) are staged in LDS; hypotheses (every pair, or pairs from
//                         sampling::distinct) are scored one after the other by the whole group (per-lane counters, one
//                         reduction per hypothesis); the refit's sums are fixed-order trees (<256>: wg::tree_sum), so a
//                         track's result is the same in any batch and in any run
//   map_threshold_kernel  LDS histogram of the track lengths and the reference's selection rule
//   map_filter_kernel     track-length and fp32 box test, ordered compaction (wg::excl_scan)
//   map_zero_kernel       the degree counts the next kernel adds to (a kernel, so that a captured call holds kernel nodes only)
//   map_adjacency_kernel  n x n closeness bits, 32 per thread; map_sweep_kernel: the reference's greedy sweep, one
//                         workgroup walking the bit rows in index order
//   map_gather_kernel     one workgroup per point, one lane per descriptor channel
// No FMA contraction: tests/mapping_oracle.py restates every expression in the same order in numpy (which never fuses),
// so every discrete outcome can be compared exactly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)   // above every project include: a shared header takes the setting of the file that includes it

#include "../../../include/mapping/mapping.h"
#include "../capi_common.h"
#include "../ransac_sample.h"
#include "../wg_primitives.h"

namespace mapk {

constexpr int CAM = 16;              // doubles per camera: [R | t] row-major 3x4, fx, fy, cx, cy
constexpr int OBS = 22;              // doubles staged per observation: the camera, the centre C, the ray d
constexpr int WG_THREADS = 256;      // the workgroup path of the triangulation
constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_THREADS) void map_verify_kernel(const float* __restrict__ kpts, const int32_t* __restrict__ kpt_offsets,
                                                                  const double* __restrict__ cams, int V,
                                                                  const int32_t* __restrict__ pair_images,
                                                                  const int32_t* __restrict__ match_offsets,
                                                                  const long long* __restrict__ matches0, double thr2, int min_inliers,
                                                                  int32_t* __restrict__ out, int32_t* __restrict__ counts) {
    __shared__ int wsum[SCAN_THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int i = pair_images[2 * p], j = pair_images[2 * p + 1];
    if (i < 0 || i >= V || j < 0 || j >= V) {   // uniform
        if (tid == 0) counts[p] = 0;
        return;
    }
    const int oi = kpt_offsets[i], oj = kpt_offsets[j];
    const int ni = kpt_offsets[i + 1] - oi, nj = kpt_offsets[j + 1] - oj;
    const int base = match_offsets[p];
    int nm = match_offsets[p + 1] - base;
    nm = nm < ni ? nm : ni;
    const double* __restrict__ ci = cams + (size_t)i * CAM;
    const double* __restrict__ cj = cams + (size_t)j * CAM;
    // relative pose R = Rj Ri^T, t = tj - R ti, essential matrix E = [t]x R
    double R[9], t[3], E[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = dot3(cj[4 * r], cj[4 * r + 1], cj[4 * r + 2], ci[4 * c], ci[4 * c + 1], ci[4 * c + 2]);
    for (int r = 0; r < 3; ++r) t[r] = cj[4 * r + 3] - dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], ci[3], ci[7], ci[11]);
    for (int c = 0; c < 3; ++c) {
        E[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
        E[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
        E[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
    }
    const double fxi = ci[12], fyi = ci[13], cxi = ci[14], cyi = ci[15];
    const double fxj = cj[12], fyj = cj[13], cxj = cj[14], cyj = cj[15];
    int run = 0;
    for (int a0 = 0; a0 < nm; a0 += SCAN_THREADS) {
        const int a = a0 + tid;
        long long b = -1;
        if (a < nm) b = matches0[(size_t)base + a];
        int keep = 0;
        if (b > -1 && b < (long long)nj) {
            const double xi = ((double)kpts[((size_t)oi + a) * 2] - cxi) / fxi, yi = ((double)kpts[((size_t)oi + a) * 2 + 1] - cyi) / fyi;
            const double xj = ((double)kpts[((size_t)oj + b) * 2] - cxj) / fxj, yj = ((double)kpts[((size_t)oj + b) * 2 + 1] - cyj) / fyj;
            const double l0 = (E[0] * xi + E[1] * yi) + E[2], l1 = (E[3] * xi + E[4] * yi) + E[5], l2 = (E[6] * xi + E[7] * yi) + E[8];
            const double k0 = (E[0] * xj + E[3] * yj) + E[6], k1 = (E[1] * xj + E[4] * yj) + E[7];
            const double num = (l0 * xj + l1 * yj) + l2;
            const double Aj = l0 / fxj, Bj = l1 / fyj, Ai = k0 / fxi, Bi = k1 / fyi;
            const double denj = Aj * Aj + Bj * Bj, deni = Ai * Ai + Bi * Bi;
            keep = denj > 0.0 && deni > 0.0 && (num * num) / denj <= thr2 && (num * num) / deni <= thr2;
        }
        int tot;
        const int pos = wg::excl_scan<SCAN_THREADS>(keep, wsum, tot);
        if (keep) {
            out[((size_t)base + run + pos) * 2] = a;
            out[((size_t)base + run + pos) * 2 + 1] = (int32_t)b;
        }
        run += tot;
    }
    if (tid == 0) counts[p] = run >= min_inliers ? run : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct TriParams {
    double thr2, cos_min;
    int max_hypotheses, refine_iterations, cap, long_cap;   // long_cap: the workgroup launch's cap, 0 when there is none
    unsigned long long seed;
};

// sums of a group of NT threads (NT = 64: the wave, shuffles; NT = 256: the workgroup, LDS), the same on every thread.
// Doubles are summed as the tree  v[t] += v[t + s], s = NT / 2 .. 1  (oracle: lane_tree_sum).
template <int NT>
struct Group {
    double* red;   // [9][NT] (NT = 256 only)
    int* redi;     // [NT]

    __device__ __forceinline__ void sync() const { __syncthreads(); }

    __device__ __forceinline__ int sum(int v) const {
        if constexpr (NT == 64) {
            return wg::wave_sum(v);
        } else {
            const int t = threadIdx.x;
            __syncthreads();
            redi[t] = v;
            __syncthreads();
            for (int s = NT / 2; s > 0; s >>= 1) {
                if (t < s) redi[t] += redi[t + s];
                __syncthreads();
            }
            return redi[0];
        }
    }

    __device__ __forceinline__ bool any(bool v) const {
        if constexpr (NT == 64) return __any(v);
        else return __syncthreads_or(v) != 0;
    }

    template <int Q>
    __device__ __forceinline__ void sum(double (&v)[Q]) const {
        if constexpr (NT == 64) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                double x = v[q];
                for (int s = 32; s > 0; s >>= 1) x += __shfl_down(x, s);
                v[q] = __shfl(x, 0);
            }
        } else {
            wg::tree_sum<NT>(v, red);
        }
    }
};

// symmetric 3x3 solve S x = b by cofactors; S = {00, 01, 02, 11, 12, 22}; false unless det > 0
__device__ __forceinline__ bool solve3(const double* S, const double* b, double* x) {
    const double c00 = S[3] * S[5] - S[4] * S[4], c01 = S[2] * S[4] - S[1] * S[5], c02 = S[1] * S[4] - S[2] * S[3];
    const double c11 = S[0] * S[5] - S[2] * S[2], c12 = S[1] * S[2] - S[0] * S[4], c22 = S[0] * S[3] - S[1] * S[1];
    const double det = (S[0] * c00 + S[1] * c01) + S[2] * c02;
    if (!(det > 0.0) || !(det < INFINITY)) return false;
    x[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
    x[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
    x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return true;
}

// the staged observations of one track, structure of arrays: o[k * cap + i], k < OBS; xy[k * cap + i], k < 2
struct Track {
    const double* o;
    const float* xy;
    int cap;
    __device__ __forceinline__ double at(int k, int i) const { return o[k * cap + i]; }

    // camera-frame point, squared reprojection error; true for an inlier
    __device__ __forceinline__ bool inlier(int i, const double* X, double thr2) const {
        const double px = dot3(at(0, i), at(1, i), at(2, i), X[0], X[1], X[2]) + at(3, i);
        const double py = dot3(at(4, i), at(5, i), at(6, i), X[0], X[1], X[2]) + at(7, i);
        const double pz = dot3(at(8, i), at(9, i), at(10, i), X[0], X[1], X[2]) + at(11, i);
        const double ex = (at(12, i) * (px / pz) + at(14, i)) - (double)xy[i];
        const double ey = (at(13, i) * (py / pz) + at(15, i)) - (double)xy[cap + i];
        return pz > 0.0 && ex * ex + ey * ey <= thr2;
    }

    // the rays from the centres of a and b to X subtend at least the minimum angle
    __device__ __forceinline__ bool angle_ok(int a, int b, const double* X, double cos_min) const {
        const double a0 = X[0] - at(16, a), a1 = X[1] - at(17, a), a2 = X[2] - at(18, a);
        const double b0 = X[0] - at(16, b), b1 = X[1] - at(17, b), b2 = X[2] - at(18, b);
        const double na = dot3(a0, a1, a2, a0, a1, a2), nb = dot3(b0, b1, b2, b0, b1, b2);
        return dot3(a0, a1, a2, b0, b1, b2) <= cos_min * sqrt(na * nb);
    }

    // midpoint of the common perpendicular of the rays of a and b; false for parallel rays
    __device__ __forceinline__ bool midpoint(int a, int b, double* X) const {
        const double Ca[3] = {at(16, a), at(17, a), at(18, a)}, da[3] = {at(19, a), at(20, a), at(21, a)};
        const double Cb[3] = {at(16, b), at(17, b), at(18, b)}, db[3] = {at(19, b), at(20, b), at(21, b)};
        const double w0 = Ca[0] - Cb[0], w1 = Ca[1] - Cb[1], w2 = Ca[2] - Cb[2];
        const double aa = dot3(da[0], da[1], da[2], da[0], da[1], da[2]), bb = dot3(da[0], da[1], da[2], db[0], db[1], db[2]);
        const double cc = dot3(db[0], db[1], db[2], db[0], db[1], db[2]);
        const double dd = dot3(da[0], da[1], da[2], w0, w1, w2), ee = dot3(db[0], db[1], db[2], w0, w1, w2);
        const double den = aa * cc - bb * bb;
        if (!(den > 0.0)) return false;
        const double s = (bb * ee - cc * dd) / den, t = (aa * ee - bb * dd) / den;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = 0.5 * ((Ca[k] + s * da[k]) + (Cb[k] + t * db[k]));
        return true;
    }
};

template <int NT>
__global__ __launch_bounds__(NT) void map_tri_kernel(const int32_t* __restrict__ track_offsets, const int32_t* __restrict__ obs_image,
                                                     const float* __restrict__ obs_xy, const double* __restrict__ cams, int V,
                                                     TriParams P, double* __restrict__ xyz, int32_t* __restrict__ mask,
                                                     int32_t* __restrict__ info, int32_t* __restrict__ lengths) {
    extern __shared__ double lds[];
    __shared__ double red[NT == 64 ? 1 : 9 * NT];
    __shared__ int redi[NT == 64 ? 1 : NT];
    const int tr = blockIdx.x, tid = threadIdx.x;
    const int o0 = track_offsets[tr];
    const int m = track_offsets[tr + 1] - o0;
    // each track belongs to exactly one of the two launches (uniform over the workgroup); without a workgroup launch the
    // wave launch reports the tracks that are longer than the caller promised
    if (NT == 64 ? m > 64 && P.long_cap > 0 : m <= 64) return;
    const int cap = P.cap;
    double* o = lds;
    float* xy = reinterpret_cast<float*>(lds + (size_t)OBS * cap);
    Group<NT> g{red, redi};
    double* out = xyz + (size_t)tr * 3;
    int32_t* I = info + (size_t)tr * 4;

    bool bad = m < 2 || m > cap;
    if (!bad) {
        bool mine = false;
        for (int i = tid; i < m; i += NT) {
            const int v = obs_image[o0 + i];
            if (v < 0 || v >= V) { mine = true; continue; }
            const double* __restrict__ c = cams + (size_t)v * CAM;
#pragma unroll
            for (int k = 0; k < CAM; ++k) o[k * cap + i] = c[k];
            const float x = obs_xy[((size_t)o0 + i) * 2], y = obs_xy[((size_t)o0 + i) * 2 + 1];
            xy[i] = x;
            xy[cap + i] = y;
            const double xn = ((double)x - c[14]) / c[12], yn = ((double)y - c[15]) / c[13];
            o[16 * cap + i] = -dot3(c[0], c[4], c[8], c[3], c[7], c[11]);
            o[17 * cap + i] = -dot3(c[1], c[5], c[9], c[3], c[7], c[11]);
            o[18 * cap + i] = -dot3(c[2], c[6], c[10], c[3], c[7], c[11]);
            o[19 * cap + i] = (c[0] * xn + c[4] * yn) + c[8];
            o[20 * cap + i] = (c[1] * xn + c[5] * yn) + c[9];
            o[21 * cap + i] = (c[2] * xn + c[6] * yn) + c[10];
        }
        bad = g.any(mine);
    }
    if (bad) {   // uniform
        for (int i = tid; i < m; i += NT) mask[o0 + i] = 0;
        if (tid < 3) out[tid] = 0.0;
        if (tid == 0) { I[0] = 0; I[1] = m; I[2] = -1; I[3] = 0; lengths[tr] = 0; }
        return;
    }
    g.sync();
    const Track T{o, xy, cap};

    // hypotheses, one after the other: every pair in lexicographic order, or hash-sampled pairs
    const long long npairs = (long long)m * (m - 1) / 2;
    const bool all_pairs = npairs <= (long long)P.max_hypotheses;
    const int H = all_pairs ? (int)npairs : P.max_hypotheses;
    int best = -1, best_cnt = 0, best_a = 0, best_b = 0;
    int a = 0, b = 0;
    for (int h = 0; h < H; ++h) {
        if (all_pairs) {
            if (++b >= m || h == 0) {
                if (h) ++a;
                b = a + 1;
            }
        } else {
            int ab[2];
            sampling::distinct(P.seed, h, m, ab);
            a = ab[0];
            b = ab[1];
        }
        double X[3];
        const bool valid = T.midpoint(a, b, X) && T.angle_ok(a, b, X, P.cos_min) && T.inlier(a, X, P.thr2) && T.inlier(b, X, P.thr2);
        if (!valid) continue;   // uniform
        int cnt = 0;
        for (int i = tid; i < m; i += NT) cnt += T.inlier(i, X, P.thr2) ? 1 : 0;
        cnt = g.sum(cnt);
        if (cnt > best_cnt) { best_cnt = cnt; best = h; best_a = a; best_b = b; }
    }
    if (best < 0) {
        for (int i = tid; i < m; i += NT) mask[o0 + i] = 0;
        if (tid < 3) out[tid] = 0.0;
        if (tid == 0) { I[0] = 0; I[1] = m; I[2] = -1; I[3] = 0; lengths[tr] = 0; }
        return;
    }
    double X[3];
    T.midpoint(best_a, best_b, X);
    // this thread's inliers of the winner: observation tid + 64 q (NT = 64: q = 0) / tid + 256 q
    unsigned inl = 0;
    for (int i = tid, q = 0; i < m; i += NT, ++q) inl |= T.inlier(i, X, P.thr2) ? 1u << q : 0u;

    // refit 1: linear least squares over the rays, sum_i (I - u u^T) X = sum_i (I - u u^T) C
    double s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.0;
    for (int i = tid, q = 0; i < m; i += NT, ++q) {
        if (!(inl >> q & 1u)) continue;
        const double d0 = T.at(19, i), d1 = T.at(20, i), d2 = T.at(21, i), C0 = T.at(16, i), C1 = T.at(17, i), C2 = T.at(18, i);
        const double n2 = dot3(d0, d1, d2, d0, d1, d2), qq = dot3(d0, d1, d2, C0, C1, C2) / n2;
        s[0] += 1.0 - d0 * d0 / n2; s[1] += -(d0 * d1 / n2); s[2] += -(d0 * d2 / n2);
        s[3] += 1.0 - d1 * d1 / n2; s[4] += -(d1 * d2 / n2); s[5] += 1.0 - d2 * d2 / n2;
        s[6] += C0 - d0 * qq; s[7] += C1 - d1 * qq; s[8] += C2 - d2 * qq;
    }
    g.sum(s);
    double Xl[3];
    if (solve3(s, s + 6, Xl)) { X[0] = Xl[0]; X[1] = Xl[1]; X[2] = Xl[2]; }

    // refit 2: Gauss-Newton on the reprojection error of the same inliers
    for (int it = 0; it < P.refine_iterations; ++it) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = 0.0;
        for (int i = tid, q = 0; i < m; i += NT, ++q) {
            if (!(inl >> q & 1u)) continue;
            const double px = dot3(T.at(0, i), T.at(1, i), T.at(2, i), X[0], X[1], X[2]) + T.at(3, i);
            const double py = dot3(T.at(4, i), T.at(5, i), T.at(6, i), X[0], X[1], X[2]) + T.at(7, i);
            const double pz = dot3(T.at(8, i), T.at(9, i), T.at(10, i), X[0], X[1], X[2]) + T.at(11, i);
            const double u = px / pz, v = py / pz;
            const double rx = (T.at(12, i) * u + T.at(14, i)) - (double)xy[i], ry = (T.at(13, i) * v + T.at(15, i)) - (double)xy[cap + i];
            const double sx = T.at(12, i) / pz, sy = T.at(13, i) / pz;
            double J0[3], J1[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                J0[k] = sx * (T.at(k, i) - u * T.at(8 + k, i));
                J1[k] = sy * (T.at(4 + k, i) - v * T.at(8 + k, i));
            }
            s[0] += J0[0] * J0[0] + J1[0] * J1[0]; s[1] += J0[0] * J0[1] + J1[0] * J1[1]; s[2] += J0[0] * J0[2] + J1[0] * J1[2];
            s[3] += J0[1] * J0[1] + J1[1] * J1[1]; s[4] += J0[1] * J0[2] + J1[1] * J1[2]; s[5] += J0[2] * J0[2] + J1[2] * J1[2];
            s[6] += J0[0] * rx + J1[0] * ry; s[7] += J0[1] * rx + J1[1] * ry; s[8] += J0[2] * rx + J1[2] * ry;
        }
        g.sum(s);
        double dx[3];
        if (!solve3(s, s + 6, dx)) break;   // uniform
        X[0] -= dx[0]; X[1] -= dx[1]; X[2] -= dx[2];
    }

    // observations that still fit, and whether two of their rays reach the minimum angle
    unsigned keep = 0;
    int cnt = 0;
    for (int i = tid, q = 0; i < m; i += NT, ++q) {
        if ((inl >> q & 1u) && T.inlier(i, X, P.thr2)) { keep |= 1u << q; ++cnt; }
    }
    cnt = g.sum(cnt);
    // publish the kept flags through the (no longer needed) fx row: every thread tests its rows against all columns
    g.sync();
    for (int i = tid, q = 0; i < m; i += NT, ++q) o[12 * cap + i] = keep >> q & 1u ? 1.0 : 0.0;
    g.sync();
    bool wide = false;
    for (int i = tid, q = 0; i < m; i += NT, ++q) {
        if (!(keep >> q & 1u)) continue;
        for (int k = i + 1; k < m; ++k) wide = wide || (T.at(12, k) != 0.0 && T.angle_ok(i, k, X, P.cos_min));
    }
    wide = g.any(wide);
    const bool ok = cnt >= 2 && wide && X[0] - X[0] == 0.0 && X[1] - X[1] == 0.0 && X[2] - X[2] == 0.0;
    for (int i = tid, q = 0; i < m; i += NT, ++q) mask[o0 + i] = ok && (keep >> q & 1u) ? 1 : 0;
    if (tid < 3) out[tid] = ok ? X[tid] : 0.0;
    if (tid == 0) { I[0] = ok; I[1] = m; I[2] = best; I[3] = best_cnt; lengths[tr] = ok ? cnt : 0; }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_THREADS) void map_threshold_kernel(const int32_t* __restrict__ lengths, int T, int max_num,
                                                                     int32_t* __restrict__ threshold) {
    __shared__ int hist[MAP_MAX_LENGTH_BINS];
    const int tid = threadIdx.x;
    for (int k = tid; k < MAP_MAX_LENGTH_BINS; k += SCAN_THREADS) hist[k] = 0;
    __syncthreads();
    for (int i = tid; i < T; i += SCAN_THREADS) {
        const int l = lengths[i];
        if (l > 0) atomicAdd(&hist[l < MAP_MAX_LENGTH_BINS ? l : MAP_MAX_LENGTH_BINS - 1], 1);
    }
    __syncthreads();
    if (tid == 0) {
        long long remaining = 0;
        for (int k = 1; k < MAP_MAX_LENGTH_BINS; ++k) remaining += hist[k];
        int thr = 0;
        for (int k = 1; k < MAP_MAX_LENGTH_BINS; ++k) {
            if (!hist[k]) continue;
            remaining -= hist[k];
            if (remaining <= (long long)max_num) { thr = k; break; }
        }
        *threshold = thr;
    }
}

struct Box {
    float c[24];
};

__global__ __launch_bounds__(SCAN_THREADS) void map_filter_kernel(const double* __restrict__ xyz, const int32_t* __restrict__ lengths, int T,
                                                                  const int32_t* __restrict__ threshold, Box B,
                                                                  int32_t* __restrict__ kept_ids, float* __restrict__ kept_xyz,
                                                                  int32_t* __restrict__ count) {
    __shared__ int wsum[SCAN_THREADS / 64];
    const int tid = threadIdx.x, thr = *threshold;
    const float* c4 = B.c + 12;
    float e[3][3], ee[3];
    const int corner[3] = {5, 0, 7};
    for (int k = 0; k < 3; ++k) {
        for (int d = 0; d < 3; ++d) e[k][d] = B.c[3 * corner[k] + d] - c4[d];
        ee[k] = (e[k][0] * e[k][0] + e[k][1] * e[k][1]) + e[k][2] * e[k][2];
    }
    int run = 0;
    for (int i0 = 0; i0 < T; i0 += SCAN_THREADS) {
        const int i = i0 + tid;
        int keep = 0;
        float p[3] = {0.0f, 0.0f, 0.0f};
        if (i < T) {
            const int l = lengths[i];
            for (int d = 0; d < 3; ++d) p[d] = (float)xyz[(size_t)i * 3 + d];
            keep = l > 0 && l >= thr;
            const float q0 = p[0] - c4[0], q1 = p[1] - c4[1], q2 = p[2] - c4[2];
            for (int k = 0; k < 3; ++k) {
                const float mm = (q0 * e[k][0] + q1 * e[k][1]) + q2 * e[k][2];
                keep = keep && 0.0f < mm && mm < ee[k];
            }
        }
        int tot;
        const int pos = wg::excl_scan<SCAN_THREADS>(keep, wsum, tot);
        if (keep) {
            kept_ids[run + pos] = i;
            for (int d = 0; d < 3; ++d) kept_xyz[(size_t)(run + pos) * 3 + d] = p[d];
        }
        run += tot;
    }
    if (tid == 0) *count = run;
}

__global__ __launch_bounds__(256) void map_zero_kernel(int* __restrict__ deg, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) deg[i] = 0;
}

// word w of row i: bit k set when point 32 w + k is closer to point i than the threshold; deg[i]: bits of row i
__global__ __launch_bounds__(256) void map_adjacency_kernel(const float* __restrict__ xyz, int n, int W, double thr,
                                                            unsigned* __restrict__ bits, int* __restrict__ deg) {
    const int w = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (w >= W) return;
    const double x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    unsigned word = 0;
    for (int k = 0; k < 32; ++k) {
        const int j = 32 * w + k;
        if (j >= n) break;
        const double dx = x - (double)xyz[(size_t)j * 3], dy = y - (double)xyz[(size_t)j * 3 + 1], dz = z - (double)xyz[(size_t)j * 3 + 2];
        if (sqrt((dx * dx + dy * dy) + dz * dz) < thr) word |= 1u << k;
    }
    bits[(size_t)i * W + w] = word;
    if (word) atomicAdd(deg + i, __popc(word));
}

__global__ __launch_bounds__(256) void map_sweep_kernel(const float* __restrict__ xyz, int n, int W, const unsigned* __restrict__ bits,
                                                        const int* __restrict__ deg, float* __restrict__ merged,
                                                        int32_t* __restrict__ member_offsets, int32_t* __restrict__ members,
                                                        int32_t* __restrict__ count) {
    __shared__ unsigned taken[MAP_MAX_POINTS / 32];
    const int tid = threadIdx.x;
    for (int w = tid; w < W; w += 256) taken[w] = 0u;
    __syncthreads();
    int n_new = 0, n_mem = 0;   // thread 0's
    for (int j = 0; j < n; ++j) {
        const unsigned* __restrict__ row = bits + (size_t)j * W;
        if (deg[j] == 1) {   // uniform; the usual row: the point alone
            if (tid == 0 && !(taken[j >> 5] >> (j & 31) & 1u)) {
                taken[j >> 5] |= 1u << (j & 31);
                for (int d = 0; d < 3; ++d) merged[(size_t)n_new * 3 + d] = __fdiv_rn(xyz[(size_t)j * 3 + d], 1.0f);
                member_offsets[n_new] = n_mem;
                members[n_mem++] = j;
                ++n_new;
            }
            __syncthreads();
            continue;
        }
        bool hit = false;
        for (int w = tid; w < W; w += 256) hit = hit || (row[w] & taken[w]) != 0u;
        if (__syncthreads_or(hit)) continue;   // a member of the row is already taken
        for (int w = tid; w < W; w += 256) taken[w] |= row[w];
        if (tid == 0) {
            float sx = 0.0f, sy = 0.0f, sz = 0.0f;
            int k = 0;
            member_offsets[n_new] = n_mem;
            for (int w = 0; w < W; ++w) {
                unsigned word = row[w];
                while (word) {
                    const int i = 32 * w + __ffs(word) - 1;
                    word &= word - 1;
                    sx += xyz[(size_t)i * 3]; sy += xyz[(size_t)i * 3 + 1]; sz += xyz[(size_t)i * 3 + 2];
                    members[n_mem++] = i;
                    ++k;
                }
            }
            merged[(size_t)n_new * 3] = __fdiv_rn(sx, (float)k);
            merged[(size_t)n_new * 3 + 1] = __fdiv_rn(sy, (float)k);
            merged[(size_t)n_new * 3 + 2] = __fdiv_rn(sz, (float)k);
            ++n_new;
        }
        __syncthreads();
    }
    if (tid == 0) {
        member_offsets[n_new] = n_mem;
        *count = n_new;
    }
}

__global__ __launch_bounds__(256) void map_gather_kernel(const float* const* __restrict__ desc_table,
                                                         const float* const* __restrict__ score_table, const int32_t* __restrict__ n_kpts,
                                                         int V, const int32_t* __restrict__ point_offsets,
                                                         const int32_t* __restrict__ obs_image, const int32_t* __restrict__ obs_kpt, int dim,
                                                         float* __restrict__ cdesc, float* __restrict__ cscores, long long* __restrict__ idxs,
                                                         double* __restrict__ mdesc, double* __restrict__ mscores) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const int k0 = point_offsets[p], k1 = point_offsets[p + 1];
    const double cnt = (double)(k1 - k0);
    for (int c = tid; c < dim; c += 256) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) {
            const int v = obs_image[k], f = obs_kpt[k];
            float x = 0.0f;
            if (v >= 0 && v < V && f >= 0 && f < n_kpts[v]) x = desc_table[v][(size_t)c * n_kpts[v] + f];
            cdesc[(size_t)k * dim + c] = x;
            s += (double)x;
        }
        mdesc[(size_t)p * dim + c] = k1 > k0 ? s / cnt : 0.0;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) {
            const int v = obs_image[k], f = obs_kpt[k];
            float x = 0.0f;
            if (v >= 0 && v < V && f >= 0 && f < n_kpts[v]) x = score_table[v][f];
            cscores[k] = x;
            s += (double)x;
        }
        mscores[p] = k1 > k0 ? s / cnt : 0.0;
        idxs[p] = (long long)(k1 - k0);
    }
}

struct Workspace {
    unsigned* bits;
    int* deg;
    size_t bytes;
};

Workspace carve(void* base, int n) {
    capi::Bump a(base);
    Workspace w;
    const size_t W = (size_t)(n + 31) / 32;
    w.bits = a.take<unsigned>((size_t)n * W * sizeof(unsigned));
    w.deg = a.take<int>((size_t)n * sizeof(int));
    w.bytes = a.off;
    return w;
}

}  // namespace mapk

using namespace mapk;
using namespace capi;

namespace {
constexpr int MAX_IMAGES = 1 << 16, MAX_PAIRS = 1 << 22, MAX_TRACKS = 1 << 24, MAX_HYPOTHESES = 1 << 16, MAX_DIM = 4096;
}

extern "C" {

int map_version(void) { return 3; }
const char* map_last_error(void) { return g_err; }

size_t map_workspace_bytes(int n_points) {
    if (n_points < 1 || n_points > MAP_MAX_POINTS) { fail(-1, "map_workspace_bytes: n_points in [1, %d] expected", MAP_MAX_POINTS); return 0; }
    return carve(nullptr, n_points).bytes;
}

int map_verify_matches(const float* kpts, const int32_t* kpt_offsets, const double* cams, int V, const int32_t* pair_images,
                       const int32_t* match_offsets, const int64_t* matches0, int P, double max_epipolar_error, int min_pair_inliers,
                       int32_t* out_matches, int32_t* counts, map_stream_t stream) {
    if (!kpts || !kpt_offsets || !cams || !pair_images || !match_offsets || !matches0 || !out_matches || !counts)
        return fail(-1, "map_verify_matches: null argument");
    if (V < 1 || V > MAX_IMAGES || P < 1 || P > MAX_PAIRS)
        return fail(-1, "map_verify_matches: V in [1, %d] and P in [1, %d] expected (got %d, %d)", MAX_IMAGES, MAX_PAIRS, V, P);
    if (!(max_epipolar_error > 0.0)) return fail(-1, "map_verify_matches: max_epipolar_error must be positive");
    hipLaunchKernelGGL(map_verify_kernel, dim3(P), dim3(SCAN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), kpts, kpt_offsets, cams, V,
                       pair_images, match_offsets, reinterpret_cast<const long long*>(matches0), max_epipolar_error * max_epipolar_error,
                       min_pair_inliers, out_matches, counts);
    return check_launch(-1, "map_verify_matches");
}

int map_triangulate_tracks(const int32_t* track_offsets, const int32_t* obs_image, const float* obs_xy, const double* cams, int T, int V,
                           int max_track_length, double max_reproj_error, double min_tri_angle_deg, int max_hypotheses,
                           int refine_iterations, uint64_t seed, double* xyz, int32_t* inlier_mask, int32_t* info, int32_t* lengths,
                           map_stream_t stream) {
    if (!track_offsets || !obs_image || !obs_xy || !cams || !xyz || !inlier_mask || !info || !lengths)
        return fail(-1, "map_triangulate_tracks: null argument");
    if (T < 1 || T > MAX_TRACKS || V < 1 || V > MAX_IMAGES)
        return fail(-1, "map_triangulate_tracks: T in [1, %d] and V in [1, %d] expected (got %d, %d)", MAX_TRACKS, MAX_IMAGES, T, V);
    if (max_track_length < 0 || max_track_length > MAP_MAX_TRACK_LENGTH)
        return fail(-1, "map_triangulate_tracks: max_track_length in [0, %d] expected (got %d)", MAP_MAX_TRACK_LENGTH, max_track_length);
    if (!(max_reproj_error > 0.0)) return fail(-1, "map_triangulate_tracks: max_reproj_error must be positive");
    if (!(min_tri_angle_deg >= 0.0) || !(min_tri_angle_deg < 180.0)) return fail(-1, "map_triangulate_tracks: min_tri_angle in [0, 180) degrees expected");
    if (max_hypotheses < 1 || max_hypotheses > MAX_HYPOTHESES || refine_iterations < 0 || refine_iterations > 1000)
        return fail(-1, "map_triangulate_tracks: max_hypotheses in [1, %d] and refine_iterations in [0, 1000] expected", MAX_HYPOTHESES);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    TriParams P;
    P.thr2 = max_reproj_error * max_reproj_error;
    P.cos_min = cos(min_tri_angle_deg * (M_PI / 180.0));
    P.max_hypotheses = max_hypotheses;
    P.refine_iterations = refine_iterations;
    P.seed = seed;
    P.cap = 64;
    P.long_cap = max_track_length > 64 ? round_up(max_track_length, 64) : 0;
    hipLaunchKernelGGL(map_tri_kernel<64>, dim3(T), dim3(64), (size_t)P.cap * (OBS * sizeof(double) + 2 * sizeof(float)), s, track_offsets,
                       obs_image, obs_xy, cams, V, P, xyz, inlier_mask, info, lengths);
    if (max_track_length > 64) {
        P.cap = round_up(max_track_length, 64);
        const size_t lds_bytes = (size_t)P.cap * (OBS * sizeof(double) + 2 * sizeof(float));
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&map_tri_kernel<WG_THREADS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes) != hipSuccess)
            return check_launch(-1, "map_triangulate_tracks");
        hipLaunchKernelGGL(map_tri_kernel<WG_THREADS>, dim3(T), dim3(WG_THREADS), lds_bytes, s, track_offsets, obs_image, obs_xy, cams, V, P, xyz, inlier_mask, info, lengths);
    }
    return check_launch(-1, "map_triangulate_tracks");
}

int map_track_length_threshold(const int32_t* lengths, int T, int max_num_kp3d, int32_t* threshold, map_stream_t stream) {
    if (!lengths || !threshold) return fail(-1, "map_track_length_threshold: null argument");
    if (T < 1 || T > MAX_TRACKS || max_num_kp3d < 0) return fail(-1, "map_track_length_threshold: T in [1, %d] and max_num_kp3d >= 0 expected", MAX_TRACKS);
    hipLaunchKernelGGL(map_threshold_kernel, dim3(1), dim3(SCAN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), lengths, T, max_num_kp3d,
                       threshold);
    return check_launch(-1, "map_track_length_threshold");
}

int map_filter_points(const double* xyz, const int32_t* lengths, int T, const int32_t* threshold, const float* box_corners_host,
                      int32_t* kept_ids, float* kept_xyz, int32_t* count, map_stream_t stream) {
    if (!xyz || !lengths || !threshold || !box_corners_host || !kept_ids || !kept_xyz || !count) return fail(-1, "map_filter_points: null argument");
    if (T < 1 || T > MAX_TRACKS) return fail(-1, "map_filter_points: T in [1, %d] expected (got %d)", MAX_TRACKS, T);
    Box B;
    memcpy(B.c, box_corners_host, sizeof(B.c));
    hipLaunchKernelGGL(map_filter_kernel, dim3(1), dim3(SCAN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz, lengths, T, threshold, B,
                       kept_ids, kept_xyz, count);
    return check_launch(-1, "map_filter_points");
}

int map_merge_points(const float* xyz32, int n, double dist_threshold, float* merged_xyz, int32_t* member_offsets, int32_t* members,
                     int32_t* count, void* workspace, size_t workspace_bytes, map_stream_t stream) {
    if (!xyz32 || !merged_xyz || !member_offsets || !members || !count) return fail(-1, "map_merge_points: null argument");
    if (n < 1 || n > MAP_MAX_POINTS) return fail(-1, "map_merge_points: n in [1, %d] expected (got %d)", MAP_MAX_POINTS, n);
    if (!(dist_threshold > 0.0)) return fail(-1, "map_merge_points: dist_threshold must be positive");
    if (!workspace) return fail(-1, "map_merge_points: null workspace");
    Workspace w = carve(workspace, n);
    if (workspace_bytes < w.bytes) return fail(-2, "map_merge_points: workspace too small: %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int W = (n + 31) / 32;
    // a kernel, not hipMemsetAsync: the memset node of a captured call wrote other values than 0 from the fifth replay of its graph on
    hipLaunchKernelGGL(map_zero_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, w.deg, n);
    hipLaunchKernelGGL(map_adjacency_kernel, dim3(ceil_div(W, 256), n), dim3(256), 0, s, xyz32, n, W, dist_threshold, w.bits, w.deg);
    hipLaunchKernelGGL(map_sweep_kernel, dim3(1), dim3(256), 0, s, xyz32, n, W, w.bits, w.deg, merged_xyz, member_offsets, members, count);
    return check_launch(-1, "map_merge_points");
}

int map_gather_descriptors(const float* const* desc_table, const float* const* score_table, const int32_t* n_kpts, int V,
                           const int32_t* point_offsets, const int32_t* obs_image, const int32_t* obs_kpt, int N, int dim,
                           float* collect_desc, float* collect_scores, int64_t* idxs, double* mean_desc, double* mean_scores,
                           map_stream_t stream) {
    if (!desc_table || !score_table || !n_kpts || !point_offsets || !obs_image || !obs_kpt || !collect_desc || !collect_scores || !idxs ||
        !mean_desc || !mean_scores)
        return fail(-1, "map_gather_descriptors: null argument");
    if (V < 1 || V > MAX_IMAGES || N < 1 || N > MAX_TRACKS || dim < 1 || dim > MAX_DIM)
        return fail(-1, "map_gather_descriptors: V in [1, %d], N in [1, %d] and dim in [1, %d] expected (got %d, %d, %d)", MAX_IMAGES,
                    MAX_TRACKS, MAX_DIM, V, N, dim);
    hipLaunchKernelGGL(map_gather_kernel, dim3(N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), desc_table, score_table, n_kpts, V,
                       point_offsets, obs_image, obs_kpt, dim, collect_desc, collect_scores, reinterpret_cast<long long*>(idxs), mean_desc,
                       mean_scores);
    return check_launch(-1, "map_gather_descriptors");
}

}  // extern "C"
