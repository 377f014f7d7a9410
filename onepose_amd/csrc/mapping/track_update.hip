// Map update step of the keyframe tracker for gfx950 (include/mapping/track_update.h): one frame's 2D-2D matches become the
// next bundle-adjustment problem.
//
// Three small latency-bound fp64 kernels, like bundle_adjust.hip: no MFMA.  Counts are integer scans and integer tree sums, no atomics of any kind;
// the per-pair arithmetic is sequential in a fixed order, so two runs are bitwise equal.  tests/track_oracle.py restates the
// arithmetic in numpy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)   // above every project include: geometry_math.h takes the setting of the file that includes it

#include "../../../include/mapping/track_update.h"
#include "../capi_common.h"
#include "../geometry_math.h"
#include "../wg_primitives.h"

namespace trk {

constexpr int WG = 1024;                            // threads of the two single-workgroup kernels
constexpr int ITEMS = TRK_MAX_KEYPOINTS / WG;       // consecutive items one of their threads owns, at most
constexpr int PAIR_THREADS = 256;
constexpr int CLS_KNOWN = 0, CLS_CANDIDATE = 1, CLS_IGNORED = 2;
constexpr int CAND_REMOVED = 0, CAND_KEPT = 1, CAND_NONFINITE = 2;
static_assert(ITEMS * WG == TRK_MAX_KEYPOINTS, "TRK_MAX_KEYPOINTS must be a multiple of the workgroup size");

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double canonical(double v) { return v != v ? quiet_nan() : v; }
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN

// what the first launch leaves for the other two
struct Ctrl {
    int m, ignored_matches;
};

// ---- per-pair geometry -----------------------------------------------------------------------------------------------------

__device__ __forceinline__ double reproj_dist(const double (&X)[3], const double* K, const double* pose, float u, float v) {
    double x, y;
    geom::project(X, K, pose, x, y);   // tracking_utils.py:74-88
    const double dx = x - (double)u, dy = y - (double)v;
    return sqrt(dx * dx + dy * dy);
}

// P = K pose[:3], row dots with the index ascending
__device__ __forceinline__ void projection_matrix(const double* __restrict__ K, const double* __restrict__ pose, double (&P)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) P[4 * r + c] = (K[3 * r] * pose[c] + K[3 * r + 1] * pose[4 + c]) + K[3 * r + 2] * pose[8 + c];
}

using geom::tri;   // geometry_math.h: the packed upper triangle geom::jacobi_eig works on

// ba_tracker.py:251-265 on one pair: view 1 sees (u1, v1), view 2 (u2, v2)
__device__ __forceinline__ void dlt(const double (&P1)[12], const double (&P2)[12], float u1, float v1, float u2, float v2, double (&X)[3]) {
    double A[4][4];
    const double x1 = (double)u1, y1 = (double)v1, x2 = (double)u2, y2 = (double)v2;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        A[0][c] = x1 * P1[8 + c] - P1[c];
        A[1][c] = y1 * P1[8 + c] - P1[4 + c];
        A[2][c] = x2 * P2[8 + c] - P2[c];
        A[3][c] = y2 * P2[8 + c] - P2[4 + c];
    }
    double S[10], V[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) S[tri<4>(a, b)] = ((A[0][a] * A[0][b] + A[1][a] * A[1][b]) + A[2][a] * A[2][b]) + A[3][a] * A[3][b];
    geom::jacobi_eig<4>(S, V, 16);
    double best = S[tri<4>(0, 0)], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (S[tri<4>(i, i)] < best) {   // ties: the lowest index stays
            best = S[tri<4>(i, i)];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = V[k][i];
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = v[k] / v[3];
}

// ---- the exact median of one workgroup's keys --------------------------------------------------------------------------------

// a double's bit pattern as an unsigned key that orders as the value does (negative values: all bits flipped; others: the sign
// bit set), and back
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b >> 63 ? ~b : b | 1ull << 63;
}
__device__ __forceinline__ double key_value(unsigned long long k) { return __longlong_as_double((long long)(k >> 63 ? k ^ 1ull << 63 : ~k)); }

// Sums over the workgroup of four counters per thread, packed as 16-bit fields of v; every total stays below 65536, so no
// field carries into the next.  wsum: WG / 64 entries of LDS.  Every thread calls it and gets the totals; it starts with a
// barrier, so two calls may follow each other on the same wsum.  The two halves step through the butterfly of wg::wave_sum
// together, in this loop of their own: as two wg::wave_sum<unsigned> calls the same instructions get other registers in
// trk_finish_kernel and trk_gate_kernel, and trk_update then measured 0.05 to 0.15 us (of 98) slower in each of three sessions.
__device__ __forceinline__ unsigned long long wg_sum4(unsigned long long v, unsigned long long* wsum) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lo += (unsigned)__shfl_xor((int)lo, d);
        hi += (unsigned)__shfl_xor((int)hi, d);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned long long)hi << 32 | lo;
    __syncthreads();
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) total += wsum[w];
    return total;
}
__device__ __forceinline__ int field(unsigned long long v, int i) { return (int)(v >> (16 * i) & 0xffffu); }

// The key of the rank-th smallest (0-based) of the values the workgroup holds: thread-private d[e] where bit e of mask is set,
// none of them NaN.  A radix select, two bits a pass from the top: a pass counts the keys that share the prefix found so far
// by their next two bits (wg_sum4: integer sums, no atomics) and every thread steps into the quarter that holds the rank.
__device__ __forceinline__ unsigned long long select_rank(const double (&d)[ITEMS], unsigned mask, int rank, unsigned long long* wsum) {
    unsigned long long prefix = 0;
#pragma unroll 1
    for (int shift = 62; shift >= 0; shift -= 2) {
        unsigned long long mine = 0;
#pragma unroll
        for (int e = 0; e < ITEMS; ++e) {
            const unsigned long long key = order_key(d[e]);
            if ((mask >> e & 1u) && (shift == 62 || (key >> (shift + 2)) == prefix)) mine += 1ull << (16 * (int)(key >> shift & 3u));
        }
        const unsigned long long all = wg_sum4(mine, wsum);
        int digit = 0;
#pragma unroll
        for (int g = 0; g < 3; ++g)
            if (digit == g && rank >= field(all, g)) {     // the four counts sum to more than rank
                rank -= field(all, g);
                ++digit;
            }
        prefix = prefix << 2 | (unsigned long long)digit;
    }
    return prefix;
}

// numpy.median of the workgroup's values (d[e] where bit e of mask is set): the middle order statistic, (a + b) / 2 of the
// two middle ones for an even count, NaN when any value is NaN or there is none.  count = how many values there are.
// Every thread of the workgroup calls it and gets the same result.
__device__ __forceinline__ double wg_median(const double (&d)[ITEMS], unsigned mask, int& count, unsigned long long* wsum) {
    unsigned long long mine = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
        if (mask >> e & 1u) mine += 1ull + (d[e] != d[e] ? 1ull << 16 : 0ull);
    const unsigned long long all = wg_sum4(mine, wsum);
    count = field(all, 0);
    if (count == 0 || field(all, 1) > 0) return quiet_nan();      // uniform over the workgroup
    const double hi = key_value(select_rank(d, mask, count / 2, wsum));
    if (count & 1) return hi;
    const double lo = key_value(select_rank(d, mask, count / 2 - 1, wsum));
    return (lo + hi) / 2.0;
}

// items [first, first + per) of n belong to thread t: consecutive, so that a scan in thread order is a scan in item order
__device__ __forceinline__ int items_per_thread(int n) { return (n + WG - 1) / WG; }

// ---- launch 1: pairs and classes ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(WG) trk_pairs_kernel(const int32_t* __restrict__ matches0, const int32_t* __restrict__ kf_pt_ids, int n_kf, int n_q,
                                                       int n_points, int32_t* __restrict__ pair_kf, int32_t* __restrict__ pair_q,
                                                       int32_t* __restrict__ q_pt_ids, double* __restrict__ pair_dist, int* __restrict__ cls,
                                                       int* __restrict__ matched, Ctrl* __restrict__ ctrl) {
    __shared__ int wsum[WG / 64];
    const int t = threadIdx.x;
    for (int j = t; j < n_q; j += WG) matched[j] = 0;
    const int per = items_per_thread(n_kf), first = t * per;
    int match[ITEMS], n_pairs = 0, n_ignored = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int i = first + e;
        match[e] = -1;
        if (e < per && i < n_kf) {
            const int v = matches0[i];
            if (v >= 0 && v < n_q) {
                match[e] = v;
                ++n_pairs;
            } else if (v != -1) {
                ++n_ignored;
            }
        }
    }
    int m, ignored;
    int k = wg::excl_scan<WG>(n_pairs, wsum, m);      // its first barrier also orders the zeroing of matched before the flags below
    (void)wg::excl_scan<WG>(n_ignored, wsum, ignored);
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
        if (match[e] >= 0) {
            const int i = first + e, id = kf_pt_ids[i];
            pair_kf[k] = i;
            pair_q[k] = match[e];
            matched[match[e]] = 1;      // two pairs may name one j: both write 1
            cls[k] = id >= 0 && id < n_points ? CLS_KNOWN : id == -1 ? CLS_CANDIDATE : CLS_IGNORED;
            ++k;
        }
    for (int r = m + t; r < n_kf; r += WG) {
        pair_kf[r] = pair_q[r] = q_pt_ids[r] = -1;
        pair_dist[2 * r] = pair_dist[2 * r + 1] = quiet_nan();
    }
    if (t == 0) {
        ctrl->m = m;
        ctrl->ignored_matches = ignored;
    }
}

// ---- launch 2: one thread per pair -------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(PAIR_THREADS) trk_geometry_kernel(const float* __restrict__ kf_xy, const float* __restrict__ q_xy,
                                                                    const int32_t* __restrict__ kf_pt_ids, const double* __restrict__ points,
                                                                    const double* __restrict__ K_kf, const double* __restrict__ K_q,
                                                                    const double* __restrict__ pose_kf, const double* __restrict__ pose_q,
                                                                    double max_reproj, double max_z, const int32_t* __restrict__ pair_kf,
                                                                    const int32_t* __restrict__ pair_q, const int* __restrict__ cls,
                                                                    const Ctrl* __restrict__ ctrl, double* __restrict__ pair_dist,
                                                                    double* __restrict__ X_all, int* __restrict__ cand) {
    const int k = blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (k >= ctrl->m) return;
    const int i = pair_kf[k], j = pair_q[k], c = cls[k];
    double d0 = quiet_nan(), d1 = quiet_nan(), X[3] = {0.0, 0.0, 0.0};
    int flag = CAND_REMOVED;
    if (c == CLS_KNOWN) {
        const int id = kf_pt_ids[i];
        const double p[3] = {points[3 * id], points[3 * id + 1], points[3 * id + 2]};
        d0 = canonical(reproj_dist(p, K_q, pose_q, q_xy[2 * j], q_xy[2 * j + 1]));
    } else if (c == CLS_CANDIDATE) {
        double P1[12], P2[12];
        projection_matrix(K_kf, pose_kf, P1);
        projection_matrix(K_q, pose_q, P2);
        dlt(P1, P2, kf_xy[2 * i], kf_xy[2 * i + 1], q_xy[2 * j], q_xy[2 * j + 1], X);
        const double rep_q = reproj_dist(X, K_q, pose_q, q_xy[2 * j], q_xy[2 * j + 1]);
        const double rep_kf = reproj_dist(X, K_kf, pose_kf, kf_xy[2 * i], kf_xy[2 * i + 1]);
        if (!(is_finite(X[0]) && is_finite(X[1]) && is_finite(X[2]) && is_finite(rep_q) && is_finite(rep_kf)))
            flag = CAND_NONFINITE;
        else if (!(rep_q > max_reproj || rep_kf > max_reproj || X[2] > max_z))
            flag = CAND_KEPT;
        d0 = canonical(rep_q);
        d1 = canonical(rep_kf);
    }
    pair_dist[2 * k] = d0;
    pair_dist[2 * k + 1] = d1;
    X_all[3 * k] = X[0];
    X_all[3 * k + 1] = X[1];
    X_all[3 * k + 2] = X[2];
    cand[k] = flag;
}

// ---- launch 3: median, gate, ids, unmatched list -----------------------------------------------------------------------------

__global__ void __launch_bounds__(WG) trk_finish_kernel(const int32_t* __restrict__ kf_pt_ids, int n_kf, int n_q, int n_points, double gate_factor,
                                                        const int32_t* __restrict__ pair_kf, const double* __restrict__ pair_dist,
                                                        const int* __restrict__ cls, const int* __restrict__ cand, const double* __restrict__ X_all,
                                                        const int* __restrict__ matched, const Ctrl* __restrict__ ctrl, int32_t* __restrict__ q_pt_ids,
                                                        double* __restrict__ new_points, int32_t* __restrict__ unmatched_q,
                                                        double* __restrict__ median, int32_t* __restrict__ summary) {
    __shared__ unsigned long long wsum4[WG / 64];
    __shared__ int wsum[WG / 64];
    const int t = threadIdx.x, m = ctrl->m;

    const int per = items_per_thread(n_kf), first = t * per;
    double d[ITEMS];
    int c[ITEMS];
    unsigned known = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int k = first + e;
        d[e] = 0.0;
        c[e] = -1;
        if (e < per && k < m) {
            c[e] = cls[k];
            if (c[e] == CLS_KNOWN) {
                d[e] = pair_dist[2 * k];
                known |= 1u << e;
            }
        }
    }
    int n_known;
    const double med = canonical(gate_factor * wg_median(d, known, n_known, wsum4));

    int n_kept = 0, n_cand = 0, n_cand_kept = 0, n_nonfinite = 0, n_bad_id = 0;
    int flag[ITEMS];
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int k = first + e;
        flag[e] = CAND_REMOVED;
        if (c[e] == CLS_KNOWN) {
            const bool keep = d[e] < med;
            q_pt_ids[k] = keep ? kf_pt_ids[pair_kf[k]] : -1;
            n_kept += keep;
        } else if (c[e] == CLS_CANDIDATE) {
            flag[e] = cand[k];
            ++n_cand;
            n_cand_kept += flag[e] == CAND_KEPT;
            n_nonfinite += flag[e] == CAND_NONFINITE;
        } else if (c[e] == CLS_IGNORED) {
            q_pt_ids[k] = -1;
            ++n_bad_id;
        }
    }
    int total_kept;
    int r = wg::excl_scan<WG>(n_cand_kept, wsum, total_kept);
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
        if (c[e] == CLS_CANDIDATE) {
            const int k = first + e;
            if (flag[e] == CAND_KEPT) {
                q_pt_ids[k] = n_points + r;
                new_points[3 * r] = X_all[3 * k];
                new_points[3 * r + 1] = X_all[3 * k + 1];
                new_points[3 * r + 2] = X_all[3 * k + 2];
                ++r;
            } else {
                q_pt_ids[k] = -1;
            }
        }
    // known kept, candidates, non-finite, ignored ids: each at most TRK_MAX_KEYPOINTS
    const unsigned long long counts = wg_sum4((unsigned long long)n_kept | (unsigned long long)n_cand << 16 | (unsigned long long)n_nonfinite << 32 |
                                                  (unsigned long long)n_bad_id << 48, wsum4);

    const int per_q = items_per_thread(n_q), first_q = t * per_q;
    int n_free = 0;
    unsigned free_mask = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int j = first_q + e;
        if (e < per_q && j < n_q && !matched[j]) {
            free_mask |= 1u << e;
            ++n_free;
        }
    }
    int n_unmatched;
    int u = wg::excl_scan<WG>(n_free, wsum, n_unmatched);
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
        if (free_mask >> e & 1u) unmatched_q[u++] = first_q + e;
    for (int j = n_unmatched + t; j < n_q; j += WG) unmatched_q[j] = -1;

    if (t == 0) {
        median[0] = med;
        summary[0] = m;
        summary[1] = n_known;
        summary[2] = field(counts, 0);
        summary[3] = field(counts, 1);
        summary[4] = total_kept;
        summary[5] = field(counts, 2);
        summary[6] = ctrl->ignored_matches + field(counts, 3);
        summary[7] = n_unmatched;
    }
}

// ---- the stage entries' kernels ----------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(PAIR_THREADS) trk_triangulate_kernel(const double* __restrict__ P1, const double* __restrict__ P2,
                                                                       const float* __restrict__ xy1, const float* __restrict__ xy2, int n,
                                                                       double* __restrict__ X_out) {
    const int k = blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (k >= n) return;
    double A[12], B[12], X[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        A[i] = P1[i];
        B[i] = P2[i];
    }
    dlt(A, B, xy1[2 * k], xy1[2 * k + 1], xy2[2 * k], xy2[2 * k + 1], X);
    X_out[3 * k] = canonical(X[0]);
    X_out[3 * k + 1] = canonical(X[1]);
    X_out[3 * k + 2] = canonical(X[2]);
}

__global__ void __launch_bounds__(WG) trk_gate_kernel(const double* __restrict__ dist, int n, double factor, double* __restrict__ median,
                                                      int32_t* __restrict__ keep) {
    __shared__ unsigned long long wsum4[WG / 64];
    const int per = items_per_thread(n), first = threadIdx.x * per;
    double d[ITEMS];
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int k = first + e;
        d[e] = 0.0;
        if (e < per && k < n) {
            d[e] = dist[k];
            mask |= 1u << e;
        }
    }
    int count;
    const double med = canonical(factor * wg_median(d, mask, count, wsum4));
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
        if (mask >> e & 1u) keep[first + e] = d[e] < med ? 1 : 0;
    if (threadIdx.x == 0) median[0] = med;
}

}  // namespace trk

using namespace trk;
using namespace capi;

namespace {

struct Workspace {
    Ctrl* ctrl;
    int *cls, *cand, *matched;
    double* X;
    size_t bytes;
};

Workspace carve(void* base, int n_kf, int n_q) {
    Bump b(base);
    Workspace w;
    w.ctrl = b.take<Ctrl>(sizeof(Ctrl));
    w.cls = b.take<int>(sizeof(int) * n_kf);
    w.cand = b.take<int>(sizeof(int) * n_kf);
    w.matched = b.take<int>(sizeof(int) * n_q);
    w.X = b.take<double>(sizeof(double) * 3 * n_kf);
    w.bytes = b.off;
    return w;
}

bool size_ok(int n) { return n >= 1 && n <= TRK_MAX_KEYPOINTS; }

int check_sizes(const char* who, int n_kf, int n_q) {
    if (!size_ok(n_kf) || !size_ok(n_q)) return fail(-1, "%s: n_kf and n_q in [1, %d] expected (got %d, %d)", who, TRK_MAX_KEYPOINTS, n_kf, n_q);
    return 0;
}

bool positive_finite(double v) { return v > 0.0 && v < INFINITY; }

}  // namespace

extern "C" {

size_t trk_workspace_bytes(int n_kf, int n_q) {
    if (check_sizes("trk_workspace_bytes", n_kf, n_q) != 0) return 0;
    return carve(nullptr, n_kf, n_q).bytes;
}

int trk_update(const int32_t* matches0, const float* kf_xy, const float* q_xy, const int32_t* kf_pt_ids, const double* points,
               const double* K_kf, const double* K_q, const double* pose_kf, const double* pose_q, int n_kf, int n_q, int n_points,
               double gate_factor, double max_reproj, double max_z, int32_t* pair_kf, int32_t* pair_q, int32_t* q_pt_ids,
               double* pair_dist, double* new_points, int32_t* unmatched_q, double* median, int32_t* summary, void* workspace,
               size_t workspace_bytes, map_stream_t stream) {
    if (!matches0 || !kf_xy || !q_xy || !kf_pt_ids || !K_kf || !K_q || !pose_kf || !pose_q || !pair_kf || !pair_q || !q_pt_ids || !pair_dist ||
        !new_points || !unmatched_q || !median || !summary)
        return fail(-1, "trk_update: null argument");
    if (int rc = check_sizes("trk_update", n_kf, n_q)) return rc;
    if (n_points < 0) return fail(-1, "trk_update: n_points >= 0 expected (got %d)", n_points);
    if (n_points > 0 && !points) return fail(-1, "trk_update: null points with n_points = %d", n_points);
    if (!positive_finite(gate_factor) || !positive_finite(max_reproj) || !positive_finite(max_z))
        return fail(-1, "trk_update: gate_factor, max_reproj and max_z must be finite and positive (got %g, %g, %g)", gate_factor, max_reproj,
                    max_z);
    if (int rc = check_workspace("trk_update", workspace, workspace_bytes, carve(nullptr, n_kf, n_q).bytes)) return rc;
    const Workspace w = carve(workspace, n_kf, n_q);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(trk_pairs_kernel, dim3(1), dim3(WG), 0, s, matches0, kf_pt_ids, n_kf, n_q, n_points, pair_kf, pair_q, q_pt_ids, pair_dist,
                       w.cls, w.matched, w.ctrl);
    hipLaunchKernelGGL(trk_geometry_kernel, dim3(ceil_div(n_kf, PAIR_THREADS)), dim3(PAIR_THREADS), 0, s, kf_xy, q_xy, kf_pt_ids, points,
                       K_kf, K_q, pose_kf, pose_q, max_reproj, max_z, pair_kf, pair_q, w.cls, w.ctrl, pair_dist, w.X, w.cand);
    hipLaunchKernelGGL(trk_finish_kernel, dim3(1), dim3(WG), 0, s, kf_pt_ids, n_kf, n_q, n_points, gate_factor, pair_kf, pair_dist, w.cls, w.cand,
                       w.X, w.matched, w.ctrl, q_pt_ids, new_points, unmatched_q, median, summary);
    return check_launch(-3, "trk_update");
}

int trk_triangulate_pairs(const double* P1, const double* P2, const float* xy1, const float* xy2, int n, double* X, map_stream_t stream) {
    if (!P1 || !P2 || !xy1 || !xy2 || !X) return fail(-1, "trk_triangulate_pairs: null argument");
    if (n < 1) return fail(-1, "trk_triangulate_pairs: n >= 1 expected (got %d)", n);
    hipLaunchKernelGGL(trk_triangulate_kernel, dim3(ceil_div(n, PAIR_THREADS)), dim3(PAIR_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), P1, P2, xy1, xy2, n, X);
    return check_launch(-3, "trk_triangulate_pairs");
}

int trk_gate_median(const double* dist, int n, double factor, double* median, int32_t* keep, void* workspace, size_t workspace_bytes,
                    map_stream_t stream) {
    if (!dist || !median || !keep) return fail(-1, "trk_gate_median: null argument");
    if (!size_ok(n)) return fail(-1, "trk_gate_median: n in [1, %d] expected (got %d)", TRK_MAX_KEYPOINTS, n);
    if (!positive_finite(factor)) return fail(-1, "trk_gate_median: factor must be finite and positive (got %g)", factor);
    if (int rc = check_workspace("trk_gate_median", workspace, workspace_bytes, carve(nullptr, n, 1).bytes)) return rc;
    hipLaunchKernelGGL(trk_gate_kernel, dim3(1), dim3(WG), 0, reinterpret_cast<hipStream_t>(stream), dist, n, factor, median, keep);
    return check_launch(-3, "trk_gate_median");
}

}  // extern "C"
