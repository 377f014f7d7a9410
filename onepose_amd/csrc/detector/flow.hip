// Flow step of the keyframe tracker (C ABI and the algorithm: include/detector/flow.h; reference: src/tracker/ba_tracker.py:113-126,
// 295-356).  Pyramidal Lucas-Kanade in fixed point: every sum over pixels is an integer (exact, order-free), the per-point
// algebra is fp64, one rounded operation at a time.  Small latency-bound work, no MFMA:
//   flow_pyr_down_kernel   one thread per pixel of the next level: 5 x 5 binomial, reflected
//   flow_track_kernel      one wave (a workgroup of its own) per point, all levels in one launch.  Per level the wave stages the
//                          (win + 3)^2 block of the first image in LDS and samples ival / ix / iy from it (Scharr on the fly), four
//                          samples to a lane in registers up to FLOW_REGISTER_SAMPLES, strided over the lanes and kept in the
//                          workspace above that; every iteration reads its four pixels per sample of the second image straight from
//                          the L2-resident level (measured faster than staging the (win + 1)^2 block in LDS: DESIGN section 18)
//                          and reduces the two mismatch sums over the wave with integer shuffles.  All branches are uniform
//                          over the wave (they hang on reduced integers), which is what allows the barriers around the staging.
//   flow_patch_kernel / flow_mismatch_kernel   the stage entries, on the same device functions
//   flow_reproj_kernel     one workgroup: mean reprojection distance with a fixed-order reduction (wg::tree_sum)
// No FMA contraction: tests/flow_oracle.py restates every expression in the same order in numpy (which never fuses), so points,
// status and trace are compared bit for bit.
#include <hip/hip_runtime.h>
#include <string.h>

#pragma clang fp contract(off)   // above every project include: geometry_math.h takes the setting of the file that includes it

#include "../../../include/detector/flow.h"
#include "../capi_common.h"
#include "../geometry_math.h"
#include "../wg_primitives.h"

namespace flow {

constexpr int MAX_LEVELS = FLOW_MAX_LEVEL + 1;
constexpr int REG_SPL = FLOW_REGISTER_SAMPLES / 64;                            // samples per lane held in registers
constexpr int MAX_SAMPLES = FLOW_MAX_WINDOW * FLOW_MAX_WINDOW;
constexpr int LDS_BYTES = (FLOW_MAX_WINDOW + 3) * (FLOW_MAX_WINDOW + 3) + 12;  // the largest staged block, 1168
constexpr double SUM_SCALE = 1.0 / 1048576.0;                                  // 2^-20
constexpr double MIN_DET = 1.0 / 8388608.0;                                    // 2^-23

struct Levels {   // by value to the kernels
    int n;
    int W[MAX_LEVELS], H[MAX_LEVELS];
    unsigned off[MAX_LEVELS];
    size_t bytes;
};

Levels make_levels(int H, int W, int n) {
    Levels lv{};
    lv.n = n;
    size_t off = 0;
    for (int l = 0; l < n; ++l) {
        lv.W[l] = W; lv.H[l] = H; lv.off[l] = (unsigned)off;
        off += (size_t)W * H;
        W = (W + 1) / 2; H = (H + 1) / 2;
    }
    lv.bytes = off;
    return lv;
}

// BORDER_REFLECT_101 (-1 -> 1, n -> n - 2), continued periodically; a 1-pixel axis maps everything to 0
__device__ __forceinline__ int reflect101(int x, int n) {
    if ((unsigned)x < (unsigned)n) return x;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    x %= p;
    if (x < 0) x += p;
    return x >= n ? p - x : x;
}

__global__ __launch_bounds__(256) void flow_pyr_down_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst, int h,
                                                            int w) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* __restrict__ row = src + (size_t)reflect101(2 * y + j - 2, H) * W;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc += k[i] * k[j] * (int)row[reflect101(2 * x + i - 2, W)];
    }
    dst[(size_t)y * w + x] = (uint8_t)((acc + 128) >> 8);
}

// steps 3-4 and the weights: the window origin of a position, the range test against the level, the bilinear weights
struct Window {
    int x, y;
    int w00, w01, w10, w11;
    bool ok;
};

__device__ __forceinline__ Window window_at(double px, double py, int win_w, int win_h, int W, int H) {
    Window w;
    const double cx = px - 0.5 * (double)(win_w - 1), cy = py - 0.5 * (double)(win_h - 1);
    const double fx = floor(cx), fy = floor(cy);
    w.ok = fx >= (double)-win_w && fx < (double)W && fy >= (double)-win_h && fy < (double)H;   // false for NaN
    w.x = w.ok ? (int)fx : 0;
    w.y = w.ok ? (int)fy : 0;
    const double a = cx - fx, b = cy - fy;
    w.w00 = (int)rint(((1.0 - a) * (1.0 - b)) * 16384.0);
    w.w01 = (int)rint((a * (1.0 - b)) * 16384.0);
    w.w10 = (int)rint(((1.0 - a) * b) * 16384.0);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// The wave copies the bw x bh block at (x0, y0) of a level into its LDS slice, reflected outside the level.  Called by the whole
// (one-wave) workgroup; the barriers order the copy against the reads before and after it.
__device__ __forceinline__ void stage_block(const uint8_t* __restrict__ img, int W, int H, int x0, int y0, int bw, int bh, uint8_t* lds,
                                            int lane) {
    __syncthreads();
    for (int i = lane; i < bw * bh; i += 64) {
        const int by = i / bw, bx = i - by * bw;
        lds[i] = img[(size_t)reflect101(y0 + by, H) * W + reflect101(x0 + bx, W)];
    }
    __syncthreads();
}

// ival / ix / iy of the samples this lane owns (sample s = 64 k + lane, row-major over the window), and where each sits in
// the window.  In registers (windows of at most FLOW_REGISTER_SAMPLES samples; a sample beyond the window holds zeros) ..
template <bool REGS>
struct PatchStore {
    short v[REG_SPL][3];
    unsigned short xy[REG_SPL];   // sy << 8 | sx
    __device__ __forceinline__ PatchStore(int16_t*, int, int, int) {}
    __device__ __forceinline__ void put(int k, int sx, int sy, bool valid, int ival, int ix, int iy) {
        v[k][0] = (short)(valid ? ival : 0); v[k][1] = (short)(valid ? ix : 0); v[k][2] = (short)(valid ? iy : 0);
        xy[k] = (unsigned short)(valid ? (sy << 8 | sx) : 0);
    }
    __device__ __forceinline__ void get(int k, int& sx, int& sy, int& ival, int& ix, int& iy) const {
        ival = v[k][0]; ix = v[k][1]; iy = v[k][2];
        sx = xy[k] & 255; sy = xy[k] >> 8;
    }
};
// .. or strided over the lanes in memory, [3][ns] int16 per point
template <>
struct PatchStore<false> {
    int16_t* mem;
    int ns, win_w, lane;
    __device__ __forceinline__ PatchStore(int16_t* m, int ns_, int win_w_, int lane_) : mem(m), ns(ns_), win_w(win_w_), lane(lane_) {}
    __device__ __forceinline__ void put(int k, int, int, bool valid, int ival, int ix, int iy) {
        const int s = k * 64 + lane;
        if (valid) { mem[s] = (int16_t)ival; mem[ns + s] = (int16_t)ix; mem[2 * ns + s] = (int16_t)iy; }
    }
    __device__ __forceinline__ void get(int k, int& sx, int& sy, int& ival, int& ix, int& iy) const {
        const int s = k * 64 + lane;
        const bool valid = s < ns;
        sy = valid ? s / win_w : 0; sx = valid ? s - sy * win_w : 0;
        ival = valid ? mem[s] : 0; ix = valid ? mem[ns + s] : 0; iy = valid ? mem[2 * ns + s] : 0;
    }
};

template <bool REGS, class F>
__device__ __forceinline__ void for_samples(int ns, F&& f) {
    if constexpr (REGS) {
#pragma unroll
        for (int k = 0; k < REG_SPL; ++k) f(k);
    } else {
        for (int k = 0; k * 64 < ns; ++k) f(k);
    }
}

// step 5: the patches of the window `w` of the first image into `store`, and A11, A12, A22 (the same on every lane)
template <bool REGS>
__device__ __forceinline__ void load_patches(const uint8_t* __restrict__ img, int W, int H, const Window& w, int win_w, int win_h,
                                             uint8_t* lds, int lane, PatchStore<REGS>& store, long long (&A)[3]) {
    const int bw = win_w + 3, ns = win_w * win_h;
    stage_block(img, W, H, w.x - 1, w.y - 1, bw, win_h + 3, lds, lane);
    int a11 = 0, a12 = 0, a22 = 0;   // at most 16 samples a lane, each product below 2^24
    for_samples<REGS>(ns, [&](int k) {
        const int s = k * 64 + lane;
        const bool valid = s < ns;
        const int sy = valid ? s / win_w : 0, sx = valid ? s - sy * win_w : 0;
        int p[4][4];   // the pixels at (w.x + sx - 1 .., w.y + sy - 1 ..)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) p[r][c] = lds[(sy + r) * bw + sx + c];
        int gx[2][2], gy[2][2];   // Scharr at the four corners; zero outside the level
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int X = w.x + sx + c, Y = w.y + sy + r;
                const bool in = (unsigned)X < (unsigned)W && (unsigned)Y < (unsigned)H;
                const int dx = 3 * (p[r][c + 2] - p[r][c]) + 10 * (p[r + 1][c + 2] - p[r + 1][c]) + 3 * (p[r + 2][c + 2] - p[r + 2][c]);
                const int dy = 3 * (p[r + 2][c] - p[r][c]) + 10 * (p[r + 2][c + 1] - p[r][c + 1]) + 3 * (p[r + 2][c + 2] - p[r][c + 2]);
                gx[r][c] = in ? dx : 0;
                gy[r][c] = in ? dy : 0;
            }
        const int ival = (p[1][1] * w.w00 + p[1][2] * w.w01 + p[2][1] * w.w10 + p[2][2] * w.w11 + 256) >> 9;
        const int ix = (gx[0][0] * w.w00 + gx[0][1] * w.w01 + gx[1][0] * w.w10 + gx[1][1] * w.w11 + 8192) >> 14;
        const int iy = (gy[0][0] * w.w00 + gy[0][1] * w.w01 + gy[1][0] * w.w10 + gy[1][1] * w.w11 + 8192) >> 14;
        store.put(k, sx, sy, valid, ival, ix, iy);
        if (valid) { a11 += ix * ix; a12 += ix * iy; a22 += iy * iy; }
    });
    A[0] = wg::wave_sum<long long>(a11); A[1] = wg::wave_sum<long long>(a12); A[2] = wg::wave_sum<long long>(a22);
}

// step 7's sums for the window `w` of the second image: B1, B2 (the same on every lane)
template <bool REGS>
__device__ __forceinline__ void mismatch(const uint8_t* __restrict__ img, int W, int H, const Window& w, int win_w, int win_h, uint8_t* lds,
                                         int lane, const PatchStore<REGS>& store, long long (&B)[2]) {
    const int ns = win_w * win_h;
#ifdef FLOW_STAGE_SECOND_IMAGE
    const int bw = win_w + 1;
    stage_block(img, W, H, w.x, w.y, bw, win_h + 1, lds, lane);
#endif
    int b1 = 0, b2 = 0;   // at most 16 samples a lane, each product below 2^25
    for_samples<REGS>(ns, [&](int k) {
        int sx, sy, ival, ix, iy;
        store.get(k, sx, sy, ival, ix, iy);
#ifndef FLOW_STAGE_SECOND_IMAGE   // the four pixels straight from the (L2-resident) level
        const int c0 = reflect101(w.x + sx, W), c1 = reflect101(w.x + sx + 1, W);
        const uint8_t* __restrict__ r0 = img + (size_t)reflect101(w.y + sy, H) * W;
        const uint8_t* __restrict__ r1 = img + (size_t)reflect101(w.y + sy + 1, H) * W;
        const int j00 = r0[c0], j01 = r0[c1], j10 = r1[c0], j11 = r1[c1];
#else   // the losing arm of the A/B in DESIGN section 18: the (win + 1)^2 block staged in the wave's LDS slice every iteration
        const uint8_t* q = lds + sy * bw + sx;
        const int j00 = q[0], j01 = q[1], j10 = q[bw], j11 = q[bw + 1];
#endif
        const int diff = ((j00 * w.w00 + j01 * w.w01 + j10 * w.w10 + j11 * w.w11 + 256) >> 9) - ival;
        b1 += diff * ix;   // ix = iy = 0 for a sample beyond the window
        b2 += diff * iy;
    });
    B[0] = wg::wave_sum<long long>(b1); B[1] = wg::wave_sum<long long>(b2);
}

template <bool REGS>
__global__ __launch_bounds__(64) void flow_track_kernel(const uint8_t* __restrict__ pyr_i, const uint8_t* __restrict__ pyr_j, Levels lv,
                                                        const float* __restrict__ pts, const float* __restrict__ init, int win_w, int win_h,
                                                        int max_iter, double eps2, double min_eig_threshold, float* __restrict__ next_pts,
                                                        int32_t* __restrict__ status, long long* __restrict__ matches0,
                                                        int32_t* __restrict__ trace, int16_t* __restrict__ patches) {
    __shared__ uint8_t lds[LDS_BYTES];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int ns = win_w * win_h;
    PatchStore<REGS> store(REGS ? nullptr : patches + (size_t)i * 3 * ns, ns, win_w, lane);
    const double px = (double)pts[2 * i], py = (double)pts[2 * i + 1];
    const double area2 = (double)(2 * win_w * win_h);
    double nx = 0.0, ny = 0.0;
    int st = 1;
    const int L = lv.n - 1;
    for (int l = L; l >= 0; --l) {
        const double scale = 1.0 / (double)(1 << l);
        const double qx = px * scale, qy = py * scale;
        if (l == L) {
            nx = (init ? (double)init[2 * i] : px) * scale;
            ny = (init ? (double)init[2 * i + 1] : py) * scale;
        } else {
            nx = 2.0 * nx;
            ny = 2.0 * ny;
        }
        const int W = lv.W[l], H = lv.H[l];
        const uint8_t* __restrict__ I = pyr_i + lv.off[l];
        const uint8_t* __restrict__ J = pyr_j + lv.off[l];
        int ran = 0, code = FLOW_EXIT_SKIPPED;
        const Window wi = window_at(qx, qy, win_w, win_h, W, H);
        if (wi.ok) {
            long long A[3];
            load_patches<REGS>(I, W, H, wi, win_w, win_h, lds, lane, store, A);
            const double a11 = (double)A[0] * SUM_SCALE, a12 = (double)A[1] * SUM_SCALE, a22 = (double)A[2] * SUM_SCALE;
            const double D = a11 * a22 - a12 * a12;
            const double min_eig = ((a22 + a11) - sqrt((a11 - a22) * (a11 - a22) + (4.0 * a12) * a12)) / area2;
            if (min_eig < min_eig_threshold || D < MIN_DET) {
                code = FLOW_EXIT_REJECTED;
            } else {
                double pdx = 0.0, pdy = 0.0;
                code = FLOW_EXIT_ITERATION_CAP;
                for (int j = 0; j < max_iter; ++j) {
                    const Window wj = window_at(nx, ny, win_w, win_h, W, H);
                    if (!wj.ok) {
                        code = FLOW_EXIT_LEFT_RANGE;
                        break;
                    }
                    ran = j + 1;
                    long long B[2];
                    mismatch<REGS>(J, W, H, wj, win_w, win_h, lds, lane, store, B);
                    const double b1 = (double)B[0] * SUM_SCALE, b2 = (double)B[1] * SUM_SCALE;
                    const double dx = (a12 * b2 - a22 * b1) / D, dy = (a12 * b1 - a11 * b2) / D;
                    nx += dx;
                    ny += dy;
                    if (dx * dx + dy * dy <= eps2) {
                        code = FLOW_EXIT_CONVERGED;
                        break;
                    }
                    if (j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
                        nx -= 0.5 * dx;
                        ny -= 0.5 * dy;
                        code = FLOW_EXIT_OSCILLATION;
                        break;
                    }
                    pdx = dx;
                    pdy = dy;
                }
            }
        }
        if (l == 0 && code >= FLOW_EXIT_LEFT_RANGE) st = 0;
        if (trace && lane == 0) {
            trace[((size_t)i * lv.n + l) * 2] = ran;
            trace[((size_t)i * lv.n + l) * 2 + 1] = code;
        }
    }
    if (st && !window_at(nx, ny, win_w, win_h, lv.W[0], lv.H[0]).ok) st = 0;   // step 8
    if (lane == 0) {
        next_pts[2 * i] = (float)nx;
        next_pts[2 * i + 1] = (float)ny;
        status[i] = st;
        matches0[i] = st ? (long long)i : -1ll;
    }
}

// stage entries: one wave per point; windows above FLOW_REGISTER_SAMPLES keep their patches in the output (patch sums) or in LDS
template <bool REGS>
__global__ __launch_bounds__(64) void flow_patch_kernel(const uint8_t* __restrict__ level, int W, int H, const double* __restrict__ pos,
                                                        int win_w, int win_h, long long* __restrict__ out_sums,
                                                        int16_t* __restrict__ out_patches) {
    __shared__ uint8_t lds[LDS_BYTES];
    const int i = blockIdx.x, lane = threadIdx.x, ns = win_w * win_h;
    int16_t* out = out_patches + (size_t)i * 3 * ns;
    PatchStore<REGS> store(out, ns, win_w, lane);
    const Window w = window_at(pos[2 * i], pos[2 * i + 1], win_w, win_h, W, H);
    long long A[3] = {0, 0, 0};
    if (w.ok) {
        load_patches<REGS>(level, W, H, w, win_w, win_h, lds, lane, store, A);
        if constexpr (REGS) {
#pragma unroll
            for (int k = 0; k < REG_SPL; ++k) {
                const int s = k * 64 + lane;
                if (s < ns) { out[s] = store.v[k][0]; out[ns + s] = store.v[k][1]; out[2 * ns + s] = store.v[k][2]; }
            }
        }
    } else {
        for (int s = lane; s < 3 * ns; s += 64) out[s] = 0;
    }
    if (lane < 3) out_sums[(size_t)i * 3 + lane] = A[lane];
}

template <bool REGS>
__global__ __launch_bounds__(64) void flow_mismatch_kernel(const uint8_t* __restrict__ level_i, const uint8_t* __restrict__ level_j, int W,
                                                           int H, const double* __restrict__ prev, const double* __restrict__ next, int win_w,
                                                           int win_h, long long* __restrict__ out_sums) {
    __shared__ uint8_t lds[LDS_BYTES];
    __shared__ int16_t held[REGS ? 1 : 3 * MAX_SAMPLES];
    const int i = blockIdx.x, lane = threadIdx.x, ns = win_w * win_h;
    PatchStore<REGS> store(held, ns, win_w, lane);
    const Window wi = window_at(prev[2 * i], prev[2 * i + 1], win_w, win_h, W, H);
    const Window wj = window_at(next[2 * i], next[2 * i + 1], win_w, win_h, W, H);
    long long A[3], B[2] = {0, 0};
    if (wi.ok && wj.ok) {
        load_patches<REGS>(level_i, W, H, wi, win_w, win_h, lds, lane, store, A);
        __syncthreads();   // the patches held in LDS
        mismatch<REGS>(level_j, W, H, wj, win_w, win_h, lds, lane, store, B);
    }
    if (lane < 2) out_sums[(size_t)i * 2 + lane] = B[lane];
}

__global__ __launch_bounds__(FLOW_REPROJ_THREADS) void flow_reproj_kernel(const double* __restrict__ pose, geom::K9 K, const float* __restrict__ X,
                                                                          const float* __restrict__ x, const int32_t* __restrict__ status,
                                                                          int n, double* __restrict__ out) {
    __shared__ double red[2 * FLOW_REPROJ_THREADS];
    const int t = threadIdx.x;
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = pose[k];
    double v[2] = {0.0, 0.0};   // sum of distances, count
    for (int i = t; i < n; i += FLOW_REPROJ_THREADS) {
        if (status[i] != 1) continue;
        const double Xi[3] = {(double)X[3 * i], (double)X[3 * i + 1], (double)X[3 * i + 2]};
        double px, py;
        geom::project(Xi, K.k, P, px, py);
        const double ex = px - (double)x[2 * i], ey = py - (double)x[2 * i + 1];
        v[0] += sqrt(ex * ex + ey * ey);
        v[1] += 1.0;
    }
    wg::tree_sum<FLOW_REPROJ_THREADS>(v, red);
    if (t == 0) {
        out[0] = v[0] / v[1];   // NaN when no point has status 1, like np.mean of nothing
        out[1] = v[1];
    }
}

}  // namespace flow

using namespace flow;
using namespace capi;

namespace {

bool window_ok(int w, int h) {
    return w >= FLOW_MIN_WINDOW && w <= FLOW_MAX_WINDOW && (w & 1) && h >= FLOW_MIN_WINDOW && h <= FLOW_MAX_WINDOW && (h & 1);
}
bool size_ok(int H, int W) { return H >= 2 && H <= FLOW_MAX_SIZE && W >= 2 && W <= FLOW_MAX_SIZE; }

int levels_for(int H, int W, int win_w, int win_h, int max_level) {
    int n = 1;
    while (n <= max_level) {
        W = (W + 1) / 2; H = (H + 1) / 2;
        if (!(W > win_w && H > win_h)) break;
        ++n;
    }
    return n;
}

size_t patch_bytes(int n, int win_w, int win_h) {
    const int ns = win_w * win_h;
    return ns > FLOW_REGISTER_SAMPLES ? (size_t)n * 3 * ns * sizeof(int16_t) : 0;
}

// 0, or the refusal of a stage entry's common arguments
int check_stage(const char* what, int H, int W, int level, int n, int win_w, int win_h) {
    if (!size_ok(H, W)) return fail(-1, "%s: H, W in [2, %d] expected (got %d, %d)", what, FLOW_MAX_SIZE, H, W);
    if (level < 0 || level > FLOW_MAX_LEVEL) return fail(-1, "%s: level in [0, %d] expected (got %d)", what, FLOW_MAX_LEVEL, level);
    if (!window_ok(win_w, win_h))
        return fail(-1, "%s: win_w, win_h odd in [%d, %d] expected (got %d, %d)", what, FLOW_MIN_WINDOW, FLOW_MAX_WINDOW, win_w, win_h);
    if (n < 0 || n > FLOW_MAX_POINTS) return fail(-1, "%s: n in [0, %d] expected (got %d)", what, FLOW_MAX_POINTS, n);
    return 0;
}

}  // namespace

extern "C" {

size_t flow_pyramid_bytes(int H, int W, int max_level) {
    if (!size_ok(H, W) || max_level < 0 || max_level > FLOW_MAX_LEVEL) {
        fail(-1, "flow_pyramid_bytes: H, W in [2, %d] and max_level in [0, %d] expected (got %d, %d, %d)", FLOW_MAX_SIZE, FLOW_MAX_LEVEL, H, W,
             max_level);
        return 0;
    }
    return make_levels(H, W, max_level + 1).bytes;
}

int flow_pyramid_levels(int H, int W, int win_w, int win_h, int max_level) {
    if (!size_ok(H, W) || max_level < 0 || max_level > FLOW_MAX_LEVEL) {
        fail(-1, "flow_pyramid_levels: H, W in [2, %d] and max_level in [0, %d] expected (got %d, %d, %d)", FLOW_MAX_SIZE, FLOW_MAX_LEVEL, H,
             W, max_level);
        return 0;
    }
    if (!window_ok(win_w, win_h)) {
        fail(-1, "flow_pyramid_levels: win_w, win_h odd in [%d, %d] expected (got %d, %d)", FLOW_MIN_WINDOW, FLOW_MAX_WINDOW, win_w, win_h);
        return 0;
    }
    return levels_for(H, W, win_w, win_h, max_level);
}

size_t flow_workspace_bytes(int n, int win_w, int win_h) {
    if (n < 0 || n > FLOW_MAX_POINTS) { fail(-1, "flow_workspace_bytes: n in [0, %d] expected (got %d)", FLOW_MAX_POINTS, n); return 0; }
    if (!window_ok(win_w, win_h)) {
        fail(-1, "flow_workspace_bytes: win_w, win_h odd in [%d, %d] expected (got %d, %d)", FLOW_MIN_WINDOW, FLOW_MAX_WINDOW, win_w, win_h);
        return 0;
    }
    return align_up(patch_bytes(n, win_w, win_h) + 1);   // never 0: that is the refusal
}

int flow_build_pyramid(const uint8_t* image_u8, int H, int W, int levels, uint8_t* pyramid, flow_stream_t stream) {
    if (!image_u8 || !pyramid) return fail(-1, "flow_build_pyramid: null argument");
    if (!size_ok(H, W)) return fail(-1, "flow_build_pyramid: H, W in [2, %d] expected (got %d, %d)", FLOW_MAX_SIZE, H, W);
    if (levels < 1 || levels > MAX_LEVELS) return fail(-1, "flow_build_pyramid: levels in [1, %d] expected (got %d)", MAX_LEVELS, levels);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const Levels lv = make_levels(H, W, levels);
    if (image_u8 != pyramid) {
        const hipError_t e = hipMemcpyAsync(pyramid, image_u8, (size_t)H * W, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return fail(-3, "flow_build_pyramid: %s", hipGetErrorString(e));
    }
    for (int l = 1; l < levels; ++l)
        hipLaunchKernelGGL(flow_pyr_down_kernel, dim3(ceil_div(lv.W[l], 64), ceil_div(lv.H[l], 4)), dim3(256), 0, s, pyramid + lv.off[l - 1],
                           lv.H[l - 1], lv.W[l - 1], pyramid + lv.off[l], lv.H[l], lv.W[l]);
    return check_launch(-3, "flow_build_pyramid");
}

int flow_patch_sums(const uint8_t* pyramid, int H, int W, int level, const double* pts64, int n, int win_w, int win_h, int64_t* out_sums,
                    int16_t* out_patches, flow_stream_t stream) {
    if (const int rc = check_stage("flow_patch_sums", H, W, level, n, win_w, win_h)) return rc;
    if (n == 0) return 0;
    if (!pyramid || !pts64 || !out_sums || !out_patches) return fail(-1, "flow_patch_sums: null argument");
    const Levels lv = make_levels(H, W, level + 1);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto* sums = reinterpret_cast<long long*>(out_sums);
    if (win_w * win_h <= FLOW_REGISTER_SAMPLES)
        hipLaunchKernelGGL(flow_patch_kernel<true>, dim3(n), dim3(64), 0, s, pyramid + lv.off[level], lv.W[level], lv.H[level], pts64, win_w,
                           win_h, sums, out_patches);
    else
        hipLaunchKernelGGL(flow_patch_kernel<false>, dim3(n), dim3(64), 0, s, pyramid + lv.off[level], lv.W[level], lv.H[level], pts64, win_w,
                           win_h, sums, out_patches);
    return check_launch(-3, "flow_patch_sums");
}

int flow_mismatch_sums(const uint8_t* pyramid_i, const uint8_t* pyramid_j, int H, int W, int level, const double* prev64,
                       const double* next64, int n, int win_w, int win_h, int64_t* out_sums, flow_stream_t stream) {
    if (const int rc = check_stage("flow_mismatch_sums", H, W, level, n, win_w, win_h)) return rc;
    if (n == 0) return 0;
    if (!pyramid_i || !pyramid_j || !prev64 || !next64 || !out_sums) return fail(-1, "flow_mismatch_sums: null argument");
    const Levels lv = make_levels(H, W, level + 1);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto* sums = reinterpret_cast<long long*>(out_sums);
    if (win_w * win_h <= FLOW_REGISTER_SAMPLES)
        hipLaunchKernelGGL(flow_mismatch_kernel<true>, dim3(n), dim3(64), 0, s, pyramid_i + lv.off[level], pyramid_j + lv.off[level],
                           lv.W[level], lv.H[level], prev64, next64, win_w, win_h, sums);
    else
        hipLaunchKernelGGL(flow_mismatch_kernel<false>, dim3(n), dim3(64), 0, s, pyramid_i + lv.off[level], pyramid_j + lv.off[level],
                           lv.W[level], lv.H[level], prev64, next64, win_w, win_h, sums);
    return check_launch(-3, "flow_mismatch_sums");
}

int flow_track(const uint8_t* pyramid_i, const uint8_t* pyramid_j, int H, int W, int levels, const float* pts, const float* init, int n,
               int win_w, int win_h, int max_iter, double eps, double min_eig_threshold, float* next_pts, int32_t* status, int64_t* matches0,
               int32_t* trace, void* workspace, size_t workspace_bytes, flow_stream_t stream) {
    if (const int rc = check_stage("flow_track", H, W, 0, n, win_w, win_h)) return rc;
    if (levels < 1 || levels > levels_for(H, W, win_w, win_h, FLOW_MAX_LEVEL))
        return fail(-1, "flow_track: levels in [1, %d] expected for a %d x %d window on %d x %d (got %d)",
                    levels_for(H, W, win_w, win_h, FLOW_MAX_LEVEL), win_w, win_h, W, H, levels);
    if (max_iter < 1 || max_iter > FLOW_MAX_ITERATIONS)
        return fail(-1, "flow_track: max_iter in [1, %d] expected (got %d)", FLOW_MAX_ITERATIONS, max_iter);
    if (!(eps >= 0.0 && eps <= 10.0)) return fail(-1, "flow_track: eps in [0, 10] expected (got %g)", eps);
    if (!(min_eig_threshold >= 0.0)) return fail(-1, "flow_track: min_eig_threshold must not be negative (got %g)", min_eig_threshold);
    if (n == 0) return 0;
    if (!pyramid_i || !pyramid_j || !pts || !next_pts || !status || !matches0) return fail(-1, "flow_track: null argument");
    if (const int rc = check_workspace("flow_track", workspace, workspace_bytes, align_up(patch_bytes(n, win_w, win_h) + 1))) return rc;
    const Levels lv = make_levels(H, W, levels);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    auto* m0 = reinterpret_cast<long long*>(matches0);
    auto* patches = static_cast<int16_t*>(workspace);
    if (win_w * win_h <= FLOW_REGISTER_SAMPLES)
        hipLaunchKernelGGL(flow_track_kernel<true>, dim3(n), dim3(64), 0, s, pyramid_i, pyramid_j, lv, pts, init, win_w, win_h, max_iter,
                           eps * eps, min_eig_threshold, next_pts, status, m0, trace, patches);
    else
        hipLaunchKernelGGL(flow_track_kernel<false>, dim3(n), dim3(64), 0, s, pyramid_i, pyramid_j, lv, pts, init, win_w, win_h, max_iter,
                           eps * eps, min_eig_threshold, next_pts, status, m0, trace, patches);
    return check_launch(-3, "flow_track");
}

int flow_reproj_mean(const double* pose, const double* K_host, const float* pts3d, const float* pts2d, const int32_t* status, int n,
                     double* out, flow_stream_t stream) {
    if (n < 0 || n > FLOW_MAX_POINTS) return fail(-1, "flow_reproj_mean: n in [0, %d] expected (got %d)", FLOW_MAX_POINTS, n);
    if (!pose || !K_host || !out || (n > 0 && (!pts3d || !pts2d || !status))) return fail(-1, "flow_reproj_mean: null argument");
    geom::K9 K;
    memcpy(K.k, K_host, sizeof(K.k));
    hipLaunchKernelGGL(flow_reproj_kernel, dim3(1), dim3(FLOW_REPROJ_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pose, K, pts3d, pts2d,
                       status, n, out);
    return check_launch(-3, "flow_reproj_mean");
}

}  // extern "C"
