// 2D object detector tail (C ABI: include/detector/detector.h; reference: src/local_feature_2D_detector/
// local_feature_2D_detector.py:85-147,160-186 and src/utils/data_utils.py:24-57,233-272).
//
// fp64 geometry on fp32 keypoints, like the reference's float64 cv2 results.  Small latency-bound work, no MFMA:
//   det_gather_kernel  one workgroup per view: ordered compaction of the valid matches into (x0, y0, x1, y1) rows
//                      (wg::excl_scan), zeroes the view's inlier mask and its best-hypothesis key
//   det_score_kernel   one wave per hypothesis (4 in turn per wave, 64 per workgroup): hash-sampled minimal set of 2
//                      (sampling::distinct) -> partial affine -> inlier count over the view's matches held as fp32 in LDS
//                      (4096-match chunks, wg::wave_sum);
//                      best kept per view as one 64-bit (count, ~index) key with a vector atomicMax
//   det_finish_kernel  one workgroup per view: mask of the winner, closed-form least-squares refit over its inliers with
//                      a fixed-order reduction (wg::tree_sum: two runs are bitwise equal), affine / info written
//   det_vote_kernel    boxes of all views and the vote
//   det_crop_kernel    the two warps of crop_img_by_bbox as one exact-integer bilinear resampling, and K_crop
// No FMA contraction: tests/detector_oracle.py restates every expression in the same order in numpy (which never fuses),
// so hypothesis counts, masks and the refit can be compared exactly.
#include <hip/hip_runtime.h>
#include <string.h>

#pragma clang fp contract(off)   // above every project include: geometry_math.h takes the setting of the file that includes it

#include "../../../include/detector/detector.h"
#include "../capi_common.h"
#include "../geometry_math.h"
#include "../ransac_sample.h"
#include "../wg_primitives.h"

namespace det {

constexpr int CHUNK = 4096;          // matches held in LDS at a time: 4096 x float4 = 64 KB
constexpr int SCORE_THREADS = 1024;  // 16 waves
constexpr int HYP_PER_WAVE = 4;
constexpr int HYP_PER_BLOCK = SCORE_THREADS / 64 * HYP_PER_WAVE;
constexpr int FIN_THREADS = 256;     // the refit's reduction order (oracle: REFIT_LANES)

struct Model {
    double a, b, tx, ty;
};

// x' = [[a, -b], [b, a]] x + t through two matches (complex division of the destination by the source difference);
// false when the two source points coincide
__device__ __forceinline__ bool model_from_pair(const float4 p, const float4 q, Model& m) {
    const double sx = (double)q.x - (double)p.x, sy = (double)q.y - (double)p.y;
    const double dx = (double)q.z - (double)p.z, dy = (double)q.w - (double)p.w;
    const double den = sx * sx + sy * sy;
    if (!(den > 0.0)) return false;
    m.a = (dx * sx + dy * sy) / den;
    m.b = (dy * sx - dx * sy) / den;
    m.tx = (double)p.z - (m.a * (double)p.x - m.b * (double)p.y);
    m.ty = (double)p.w - (m.b * (double)p.x + m.a * (double)p.y);
    return true;
}

__device__ __forceinline__ bool hypothesis(const float4* __restrict__ pts, int n, unsigned long long seed, int hyp, Model& m) {
    int idx[2];
    sampling::distinct(seed, hyp, n, idx);   // n >= 2
    return model_from_pair(pts[idx[0]], pts[idx[1]], m);
}

__device__ __forceinline__ double residual2(const Model& m, const float4 p) {
    const double x = p.x, y = p.y;
    const double ex = ((m.a * x - m.b * y) + m.tx) - (double)p.z;
    const double ey = ((m.b * x + m.a * y) + m.ty) - (double)p.w;
    return ex * ex + ey * ey;
}

// local_feature_2D_detector.py:85-90 on the device; matches0 == nullptr: kpts0 / kpts1 are point lists of n_host pairs
__global__ __launch_bounds__(1024) void det_gather_kernel(const float* __restrict__ kpts0, const int32_t* __restrict__ n0,
                                                          const long long* __restrict__ matches0, const float* __restrict__ kpts1,
                                                          int cap0, int n1, int n_host, float4* __restrict__ pts_all,
                                                          int* __restrict__ src_all, int* __restrict__ count,
                                                          unsigned long long* __restrict__ best, int32_t* __restrict__ mask_all) {
    __shared__ int wsum[16];
    const int v = blockIdx.x, tid = threadIdx.x;
    const size_t base_v = (size_t)v * cap0;
    int n = n0 ? n0[v] : n_host;
    n = n < 0 ? 0 : (n > cap0 ? cap0 : n);
    int run = 0;
    for (int i0 = 0; i0 < cap0; i0 += 1024) {
        const int i = i0 + tid;
        long long m = -1;
        if (i < n) m = matches0 ? matches0[base_v + i] : (long long)i;
        const int valid = m > -1 && m < (long long)n1;
        if (i < cap0) mask_all[base_v + i] = 0;
        int tot;
        const int pos = wg::excl_scan<1024>(valid, wsum, tot);
        if (valid) {
            const int o = run + pos;
            pts_all[base_v + o] = make_float4(kpts0[(base_v + i) * 2], kpts0[(base_v + i) * 2 + 1], kpts1[(size_t)m * 2],
                                              kpts1[(size_t)m * 2 + 1]);
            src_all[base_v + o] = i;
        }
        run += tot;
    }
    if (tid == 0) {
        count[v] = run;
        best[v] = 0ull;
    }
}

__global__ __launch_bounds__(SCORE_THREADS) void det_score_kernel(const float4* __restrict__ pts_all, const int* __restrict__ count,
                                                                  int cap0, int min_matches, double thr2, int iterations,
                                                                  unsigned long long seed, unsigned long long* __restrict__ best) {
    __shared__ float4 lds[CHUNK];
    const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = count[v];
    if (n < min_matches) return;   // uniform over the workgroup
    const float4* __restrict__ pts = pts_all + (size_t)v * cap0;
    const int h0 = blockIdx.x * HYP_PER_BLOCK + wave * HYP_PER_WAVE;
    Model m[HYP_PER_WAVE];
    bool valid[HYP_PER_WAVE];
    int cnt[HYP_PER_WAVE];
#pragma unroll
    for (int k = 0; k < HYP_PER_WAVE; ++k) {
        cnt[k] = 0;
        m[k] = Model{0.0, 0.0, 0.0, 0.0};
        valid[k] = h0 + k < iterations && hypothesis(pts, n, seed, h0 + k, m[k]);
    }
    for (int c0 = 0; c0 < n; c0 += CHUNK) {
        const int cn = n - c0 < CHUNK ? n - c0 : CHUNK;
        __syncthreads();
        for (int i = tid; i < cn; i += SCORE_THREADS) lds[i] = pts[c0 + i];
        __syncthreads();
        for (int i = lane; i < cn; i += 64) {
            const float4 p = lds[i];
#pragma unroll
            for (int k = 0; k < HYP_PER_WAVE; ++k) cnt[k] += residual2(m[k], p) <= thr2 ? 1 : 0;
        }
    }
    unsigned long long key = 0ull;
#pragma unroll
    for (int k = 0; k < HYP_PER_WAVE; ++k) {
        const int c = wg::wave_sum(cnt[k]);
        if (valid[k]) {
            const unsigned long long kk = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(~(unsigned)(h0 + k));
            key = kk > key ? kk : key;
        }
    }
    if (lane == 0 && key != 0ull) atomicMax(best + v, key);
}

__global__ __launch_bounds__(FIN_THREADS) void det_finish_kernel(const float4* __restrict__ pts_all, const int* __restrict__ src_all,
                                                                 const int* __restrict__ count,
                                                                 const unsigned long long* __restrict__ best, int cap0,
                                                                 int min_matches, double thr2, unsigned long long seed,
                                                                 double* __restrict__ affine, int32_t* __restrict__ mask_all,
                                                                 int32_t* __restrict__ info) {
    __shared__ double red[4 * FIN_THREADS];
    __shared__ int redc[FIN_THREADS];
    const int v = blockIdx.x, t = threadIdx.x;
    const int n = count[v];
    const unsigned long long key = best[v];
    const float4* __restrict__ pts = pts_all + (size_t)v * cap0;
    const int* __restrict__ src = src_all + (size_t)v * cap0;
    int32_t* __restrict__ mask = mask_all + (size_t)v * cap0;
    double* A = affine + (size_t)v * 6;
    int32_t* I = info + (size_t)v * 4;
    Model m{0.0, 0.0, 0.0, 0.0};
    const int hyp = (int)(~(unsigned)(key & 0xffffffffull));
    const bool ok = n >= min_matches && key != 0ull && hypothesis(pts, n, seed, hyp, m);   // uniform
    if (!ok) {
        if (t < 6) A[t] = 0.0;
        if (t == 0) { I[0] = 0; I[1] = n; I[2] = -1; I[3] = 0; }
        return;
    }
    // pass 1: mask of the winner, centroids of its inliers
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int c = 0;
    for (int i = t; i < n; i += FIN_THREADS) {
        const float4 p = pts[i];
        if (residual2(m, p) <= thr2) {
            mask[src[i]] = 1;
            s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z; s[3] += (double)p.w;
            ++c;
        }
    }
    redc[t] = c;
    wg::tree_sum<FIN_THREADS>(s, red);
    if (t == 0) {
        int tot = 0;
        for (int i = 0; i < FIN_THREADS; ++i) tot += redc[i];
        redc[0] = tot;
    }
    __syncthreads();
    const int n_inl = redc[0];
    const double cnt = (double)n_inl;
    const double csx = s[0] / cnt, csy = s[1] / cnt, cdx = s[2] / cnt, cdy = s[3] / cnt;
    // pass 2: centred sums
    double u[3] = {0.0, 0.0, 0.0};   // sums of |u|^2, u . w, u x w
    for (int i = t; i < n; i += FIN_THREADS) {
        const float4 p = pts[i];
        if (residual2(m, p) <= thr2) {
            const double ux = (double)p.x - csx, uy = (double)p.y - csy, wx = (double)p.z - cdx, wy = (double)p.w - cdy;
            u[0] += ux * ux + uy * uy;
            u[1] += ux * wx + uy * wy;
            u[2] += ux * wy - uy * wx;
        }
    }
    wg::tree_sum<FIN_THREADS>(u, red);
    if (t == 0) {
        const double den = u[0];
        if (!(den > 0.0)) {   // cannot happen after a non-degenerate sample; never divide by zero
            for (int k = 0; k < 6; ++k) A[k] = 0.0;
            I[0] = 0; I[1] = n; I[2] = -1; I[3] = 0;
        } else {
            const double a = u[1] / den, b = u[2] / den;
            A[0] = a; A[1] = -b; A[2] = cdx - (a * csx - b * csy);
            A[3] = b; A[4] = a;  A[5] = cdy - (b * csx + a * csy);
            I[0] = 1; I[1] = n; I[2] = hyp; I[3] = n_inl;
        }
    }
}

__device__ __forceinline__ int trunc_i32(double x) {   // .astype(np.int32): toward zero; clamped (numpy: undefined out of range)
    if (!(x > -2147483648.0)) return INT32_MIN;
    if (!(x < 2147483647.0)) return INT32_MAX;
    return (int)x;
}

__device__ void view_box(const double* __restrict__ A, const int32_t* __restrict__ I, const int32_t* __restrict__ hw, int qh, int qw,
                         int (&box)[4]) {
    if (!I[0]) {   // :96-99: [0, 0, size[0], size[1]] with size = (H, W)
        box[0] = 0; box[1] = 0; box[2] = qh; box[3] = qw;
        return;
    }
    const double H0 = hw[0], W0 = hw[1];
    const double cx[4] = {0.0, W0, 0.0, W0}, cy[4] = {0.0, 0.0, H0, H0};
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
    for (int k = 0; k < 4; ++k) {
        const int px = trunc_i32((A[0] * cx[k] + A[1] * cy[k]) + A[2]);
        const int py = trunc_i32((A[3] * cx[k] + A[4] * cy[k]) + A[5]);
        x0 = px < x0 ? px : x0; x1 = px > x1 ? px : x1;
        y0 = py < y0 ? py : y0; y1 = py > y1 ? py : y1;
    }
    box[0] = x0; box[1] = y0; box[2] = x1; box[3] = y1;
}

__global__ __launch_bounds__(256) void det_vote_kernel(const double* __restrict__ affine, const int32_t* __restrict__ info,
                                                       const int32_t* __restrict__ hw0, int V, int qh, int qw, int rank_by,
                                                       int32_t* __restrict__ boxes, int32_t* __restrict__ bbox,
                                                       int32_t* __restrict__ best_view) {
    for (int v = threadIdx.x; v < V; v += 256) {
        int box[4];
        view_box(affine + (size_t)v * 6, info + (size_t)v * 4, hw0 + (size_t)v * 2, qh, qw, box);
        for (int k = 0; k < 4; ++k) boxes[(size_t)v * 4 + k] = box[k];
    }
    if (threadIdx.x == 0) {   // :139-147: stable sort, descending: the first view with the largest key
        int bv = 0, bk = -1;
        for (int v = 0; v < V; ++v) {
            const int32_t* I = info + (size_t)v * 4;
            const int k = I[0] ? (rank_by == DET_RANK_BY_INLIERS ? I[3] : I[1]) : 0;
            if (k > bk) { bk = k; bv = v; }
        }
        int box[4];
        view_box(affine + (size_t)bv * 6, info + (size_t)bv * 4, hw0 + (size_t)bv * 2, qh, qw, box);
        for (int k = 0; k < 4; ++k) bbox[k] = box[k];
        *best_view = bv;
    }
}

__global__ __launch_bounds__(256) void det_crop_kernel(const uint8_t* __restrict__ img, int H, int W, const int32_t* __restrict__ bbox,
                                                       geom::K9 K, int crop, int log2crop, float* __restrict__ out,
                                                       double* __restrict__ K_crop, int32_t* __restrict__ info) {
    const long long x0 = bbox[0], y0 = bbox[1];
    const long long w = (long long)bbox[2] - x0, h = (long long)bbox[3] - y0;
    const bool ok = w > 0 && h > 0;
    const int u = blockIdx.x * 64 + (threadIdx.x & 63), vv = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        info[0] = ok; info[3] = 0;
        info[1] = (int32_t)(w > INT32_MAX ? INT32_MAX : (w < INT32_MIN ? INT32_MIN : w));
        info[2] = (int32_t)(h > INT32_MAX ? INT32_MAX : (h < INT32_MIN ? INT32_MIN : h));
        if (ok) {   // K_crop = M2 M1 K, M2 M1 = [[s, 0, -s x0], [0, s, crop / 2 - s h / 2 - s y0], [0, 0, 1]]
            const double s = (double)crop / (double)w;
            const double m02 = -(s * (double)x0);
            const double m12 = (0.5 * (double)crop - s * (0.5 * (double)h)) - s * (double)y0;
            for (int j = 0; j < 3; ++j) {
                K_crop[j] = s * K.k[j] + m02 * K.k[6 + j];
                K_crop[3 + j] = s * K.k[3 + j] + m12 * K.k[6 + j];
                K_crop[6 + j] = K.k[6 + j];
            }
        } else {
            for (int j = 0; j < 9; ++j) K_crop[j] = 0.0;
        }
    }
    if (u >= crop || vv >= crop) return;
    float val = 0.0f;
    if (ok) {
        // sampling position in the w x h crop, in units of 1 / crop
        const long long Xs = (long long)u * w, Ys = (long long)(vv - crop / 2) * w + h * (long long)(crop / 2);
        const long long ix = Xs >> log2crop, iy = Ys >> log2crop;   // floor
        const int fx = (int)(Xs & (crop - 1)), fy = (int)(Ys & (crop - 1));
        int p[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const long long x = ix + dx, y = iy + dy;
                const long long X = x + x0, Y = y + y0;
                const bool in = x >= 0 && x < w && y >= 0 && y < h && X >= 0 && X < W && Y >= 0 && Y < H;
                p[dy][dx] = in ? (int)img[(size_t)Y * W + (size_t)X] : 0;
            }
        const int sum = (crop - fx) * (crop - fy) * p[0][0] + fx * (crop - fy) * p[0][1] + (crop - fx) * fy * p[1][0] + fx * fy * p[1][1];
        const int sh = 2 * log2crop;
        int q = sum >> sh;
        const int r = sum & ((1 << sh) - 1), half = 1 << (sh - 1);
        if (r > half || (r == half && (q & 1))) ++q;   // round half to even
        val = __fdiv_rn((float)q, 255.0f);
    }
    out[(size_t)vv * crop + u] = val;
}

struct Workspace {
    float4* pts;
    int* src;
    unsigned long long* best;
    int* count;
    size_t bytes;
};

Workspace carve(void* base, int V, int cap0) {
    capi::Bump a(base);
    Workspace w;
    w.pts = a.take<float4>((size_t)V * cap0 * sizeof(float4));
    w.src = a.take<int>((size_t)V * cap0 * sizeof(int));
    w.best = a.take<unsigned long long>((size_t)V * sizeof(unsigned long long));
    w.count = a.take<int>((size_t)V * sizeof(int));
    w.bytes = a.off;
    return w;
}

}  // namespace det

using namespace det;
using namespace capi;

namespace {
constexpr int MAX_VIEWS = 4096, MAX_CAP0 = 1 << 20, MAX_ITERATIONS = 1 << 24;
bool shape_ok(int V, int cap0, int iterations) {
    return V >= 1 && V <= MAX_VIEWS && cap0 >= 1 && cap0 <= MAX_CAP0 && iterations >= 1 && iterations <= MAX_ITERATIONS;
}

int ransac(const float* kpts0, const int32_t* n0, const int64_t* matches0, const float* kpts1, int V, int cap0, int n1, int n_host,
           int min_matches, double thr, int iterations, uint64_t seed, double* affine, int32_t* mask, int32_t* info, void* workspace,
           size_t workspace_bytes, det_stream_t stream, const char* what) {
    if (!shape_ok(V, cap0, iterations))
        return fail(-1, "%s: V in [1, %d], cap0 / n in [1, %d] and iterations in [1, %d] expected (got %d, %d, %d)", what, MAX_VIEWS,
                    MAX_CAP0, MAX_ITERATIONS, V, cap0, iterations);
    if (!(thr > 0.0)) return fail(-1, "%s: reproj_threshold must be positive", what);
    if (!workspace) return fail(-1, "%s: null workspace", what);
    Workspace w = carve(workspace, V, cap0);
    if (workspace_bytes < w.bytes) return fail(-2, "%s: workspace too small: %zu < %zu bytes", what, workspace_bytes, w.bytes);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const double thr2 = thr * thr;
    hipLaunchKernelGGL(det_gather_kernel, dim3(V), dim3(1024), 0, s, kpts0, n0, reinterpret_cast<const long long*>(matches0), kpts1, cap0,
                       n1, n_host, w.pts, w.src, w.count, w.best, mask);
    hipLaunchKernelGGL(det_score_kernel, dim3(ceil_div(iterations, HYP_PER_BLOCK), V), dim3(SCORE_THREADS), 0, s, w.pts,
                       w.count, cap0, min_matches, thr2, iterations, (unsigned long long)seed, w.best);
    hipLaunchKernelGGL(det_finish_kernel, dim3(V), dim3(FIN_THREADS), 0, s, w.pts, w.src, w.count, w.best, cap0, min_matches, thr2,
                       (unsigned long long)seed, affine, mask, info);
    return check_launch(-1, what);
}
}  // namespace

extern "C" {

int det_version(void) { return 2; }   // 2: the flow step (flow.hip, include/detector/flow.h) joined the library
const char* det_last_error(void) { return g_err; }

size_t det_workspace_bytes(int V, int cap0, int iterations) {
    if (!shape_ok(V, cap0, iterations)) { fail(-1, "det_workspace_bytes: shape out of range"); return 0; }
    return carve(nullptr, V, cap0).bytes;
}

int det_affine_partial_ransac(const float* src, const float* dst, int n, double reproj_threshold, int iterations, uint64_t seed,
                              double* affine, int32_t* inlier_mask, int32_t* info, void* workspace, size_t workspace_bytes,
                              det_stream_t stream) {
    if (!src || !dst || !affine || !inlier_mask || !info) return fail(-1, "det_affine_partial_ransac: null argument");
    return ransac(src, nullptr, nullptr, dst, 1, n, n, n, 2, reproj_threshold, iterations, seed, affine, inlier_mask, info, workspace,
                  workspace_bytes, stream, "det_affine_partial_ransac");
}

int det_affine_partial_from_matches(const float* kpts0, const int32_t* n0, const int64_t* matches0, const float* kpts1, int V, int cap0,
                                    int n1, double reproj_threshold, int iterations, uint64_t seed, double* affine, int32_t* inlier_mask,
                                    int32_t* info, void* workspace, size_t workspace_bytes, det_stream_t stream) {
    if (!kpts0 || !n0 || !matches0 || !affine || !inlier_mask || !info) return fail(-1, "det_affine_partial_from_matches: null argument");
    if (n1 < 0 || (n1 > 0 && !kpts1)) return fail(-1, "det_affine_partial_from_matches: n1 must be >= 0 and kpts1 non-null when n1 > 0");
    return ransac(kpts0, n0, matches0, kpts1, V, cap0, n1, 0, DET_MIN_MATCHES, reproj_threshold, iterations, seed, affine, inlier_mask,
                  info, workspace, workspace_bytes, stream, "det_affine_partial_from_matches");
}

int det_bbox_vote(const double* affine, const int32_t* info, const int32_t* hw0, int V, int query_h, int query_w, int rank_by,
                  int32_t* boxes, int32_t* bbox, int32_t* best_view, det_stream_t stream) {
    if (!affine || !info || !hw0 || !boxes || !bbox || !best_view) return fail(-1, "det_bbox_vote: null argument");
    if (V < 1 || V > MAX_VIEWS) return fail(-1, "det_bbox_vote: V in [1, %d] expected (got %d)", MAX_VIEWS, V);
    if (rank_by != DET_RANK_BY_MATCHES && rank_by != DET_RANK_BY_INLIERS) return fail(-1, "det_bbox_vote: unknown rank_by %d", rank_by);
    if (query_h < 1 || query_w < 1) return fail(-1, "det_bbox_vote: query size must be positive");
    hipLaunchKernelGGL(det_vote_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), affine, info, hw0, V, query_h,
                       query_w, rank_by, boxes, bbox, best_view);
    return check_launch(-1, "det_bbox_vote");
}

int det_crop_resize(const uint8_t* image_u8, int H, int W, const int32_t* bbox, const double* K_host, int crop_size, float* out,
                    double* K_crop, int32_t* info, det_stream_t stream) {
    if (!image_u8 || !bbox || !K_host || !out || !K_crop || !info) return fail(-1, "det_crop_resize: null argument");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 31)) return fail(-1, "det_crop_resize: image size out of range");
    if (crop_size < 2 || crop_size > 2048 || (crop_size & (crop_size - 1)))
        return fail(-1, "det_crop_resize: crop_size must be a power of two in [2, 2048] (got %d): the exact-integer resampling needs it",
                    crop_size);
    int lg = 0;
    while ((1 << lg) < crop_size) ++lg;
    geom::K9 K;
    memcpy(K.k, K_host, sizeof(K.k));
    hipLaunchKernelGGL(det_crop_kernel, dim3(ceil_div(crop_size, 64), ceil_div(crop_size, 4)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), image_u8, H, W, bbox, K, crop_size, lg, out, K_crop, info);
    return check_launch(-1, "det_crop_resize");
}

}  // extern "C"
