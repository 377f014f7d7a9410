// SuperGlue 2D-2D matcher on gfx950 (include/superglue/superglue.h): keypoint encoder, attentional GNN,
// log-space Sinkhorn and match tail.  fp32 throughout: the GEMMs and the attention run on
// v_mfma_f32_32x32x2_f32, everything else on fp32 VALU.
//
// Channel-major activations as in the reference ([b][C][n] per side).  Every reduction runs in a fixed
// order (no atomics), so two calls on the same inputs are bitwise identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../../include/superglue/superglue.h"
#include "../capi_common.h"

namespace {

using namespace capi;

constexpr int D = SG_DESC_DIM;
constexpr int KENC[6] = {3, 32, 64, 128, 256, 256};
constexpr float BN_EPS = 1e-5f;

// ---------------------------------------------------------------------------------------------------------------------
// Packed weight layout (floats).  BatchNorm parameters are packed as [4][C]: running_mean, running_var, gamma, beta.
// q / k / v rows and merge columns are head-contiguous: packed channel h*64 + d is reference channel d*4 + h.
// ---------------------------------------------------------------------------------------------------------------------
struct KencOff {
    size_t w[5], b[5], bn[4];
};
constexpr size_t OFF_BIN = 0;
constexpr size_t KENC_BASE = 4;

KencOff kenc_offsets() {
    KencOff o{};
    size_t p = KENC_BASE;
    for (int l = 0; l < 5; ++l) {
        o.w[l] = p; p += size_t(KENC[l + 1]) * KENC[l];
        o.b[l] = p; p += KENC[l + 1];
        if (l < 4) { o.bn[l] = p; p += 4 * size_t(KENC[l + 1]); }
    }
    return o;
}
constexpr size_t KENC_FLOATS = (96 + 32 + 128) + (2048 + 64 + 256) + (8192 + 128 + 512) + (32768 + 256 + 1024) + (65536 + 256);
constexpr size_t L_WQKV = 0, L_BQKV = L_WQKV + 3 * D * D, L_WM = L_BQKV + 3 * D, L_BM = L_WM + D * D, L_W1 = L_BM + D,
                 L_B1 = L_W1 + 2 * D * 2 * D, L_BN1 = L_B1 + 2 * D, L_W2 = L_BN1 + 4 * 2 * D, L_B2 = L_W2 + D * 2 * D,
                 LAYER_FLOATS = L_B2 + D;
size_t layer_base(int l) { return KENC_BASE + KENC_FLOATS + size_t(l) * LAYER_FLOATS; }
size_t final_base(int n_layers) { return layer_base(n_layers); }
size_t packed_floats(int n_layers) { return final_base(n_layers) + D * D + D; }

// ---------------------------------------------------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

// row (within a 32x32 MFMA tile) held by accumulator register r of a lane in half `half`
__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ int head_perm(int i) { return (i & 63) * 4 + (i >> 6); }   // packed channel -> reference channel

// dst[r][c] = src[pr(r)][pc(c)], pr / pc the head permutation where asked
__global__ void sg_copy_perm_kernel(float* dst, const float* src, int rows, int cols, int perm_rows, int perm_cols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i % cols;
    const int sr = perm_rows ? head_perm(r) : r, sc = perm_cols ? head_perm(c) : c;
    dst[i] = src[size_t(sr) * cols + sc];
}

// ---- per-item counts ----
// A batch is b items; item i matches n[0][i] points of side 0 against n[1][i] points of side 1.  The table travels by value in
// the kernel arguments (the library copies nothing from host memory), so every lookup is a scalar load at a block-uniform
// index.  A uniform batch (sg_forward: one n0, one n1, any b) is the table with `uniform` set and entry 0 filled.  Buffers
// are laid out by the capacities (cap0, cap1); a kernel bounds its loops, masks and stores by the item's own counts, so the
// order of every reduction depends on the item alone and nothing past an item's counts is ever read.
struct Items {
    int n[2][SG_MAX_ITEMS];
    int uniform;
    __host__ __device__ int slot(int bi) const { return uniform ? 0 : bi; }
    __host__ __device__ int count(int s, int bi) const { return n[s][slot(bi)]; }
};
struct Marginals {   // log_optimal_transport's (:157-165), per item, computed on the host
    float norm[SG_MAX_ITEMS], mu_last[SG_MAX_ITEMS], nu_last[SG_MAX_ITEMS];
};

// ---- fp32 MFMA GEMM: C[m][n] = epilogue( sum_k A[m][k] B[k][n] ), 64x64 tiles, 4 waves of 32x32, K slabs of 32 ----
struct GemmJob {
    const float* A; long sA;          // row-major [M][K] (lda) or, with a_km, [K][M] (lda); batch stride sA
    const float* bias;                // [M] or null
    const float* bn;                  // [4][M] (mean, var, gamma, beta) or null
    const float* B; long sB;          // [K][N] for k < ksplit
    const float* B2; long sB2;        // [K - ksplit][N] for k >= ksplit (the cat(x, message) operand; no concatenation)
    float* C; long sC; int ldc;
    float* Ct; long sCt; int ldct;    // optional transposed copy: Ct[n][m]
    const float* R; long sR;          // optional residual (ld = ldc): C = R + epilogue
    int M, N;                         // capacities: N is the leading dimension of B / B2
    int msel, nsel;                   // rows / columns of an item: count(msel) (M itself if msel < 0), count(nsel)
};
struct GemmArgs {
    GemmJob job[4];
    int njobs, b, K, ksplit, lda, a_km, relu;
    float scale;                      // applied to the accumulator first (1 = none)
    Items items;
};

__global__ __launch_bounds__(256) void sg_gemm_kernel(GemmArgs p) {
    const int jz = blockIdx.z / p.b, bi = blockIdx.z % p.b;
    const GemmJob& J = p.job[jz];
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int M = J.msel < 0 ? J.M : p.items.count(J.msel, bi), N = p.items.count(J.nsel, bi);
    if (m0 >= M || n0 >= N) return;
    const float* A = J.A + bi * J.sA;
    const float* B = J.B + bi * J.sB;
    const float* B2 = J.B2 ? J.B2 + bi * J.sB2 : nullptr;
    const int K = p.K, lda = p.lda, ldb = J.N;

    __shared__ float As[32][64 + 4];
    __shared__ float Bs[32][64 + 4];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, half = l >> 5, c = l & 31;
    const int wm = w & 1, wn = w >> 1;

    float ra[8], rb[8];
    auto load = [&](int kt) {
        const int k0 = kt * 32;
        if (p.a_km) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kk = (tid >> 6) + 4 * i, m = tid & 63;
                ra[i] = (m0 + m < M) ? A[size_t(k0 + kk) * lda + m0 + m] : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i, m = idx >> 3, kq = (idx & 7) * 4;
                const float4 v = *reinterpret_cast<const float4*>(A + size_t(m0 + m) * lda + k0 + kq);
                ra[4 * i + 0] = v.x; ra[4 * i + 1] = v.y; ra[4 * i + 2] = v.z; ra[4 * i + 3] = v.w;
            }
        }
        const bool second = k0 >= p.ksplit;
        const float* Bp = second ? B2 + size_t(k0 - p.ksplit) * ldb : B + size_t(k0) * ldb;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = (tid >> 6) + 4 * i, n = tid & 63;
            rb[i] = (n0 + n < N) ? Bp[size_t(kk) * ldb + n0 + n] : 0.f;
        }
    };
    auto store = [&]() {
        if (p.a_km) {
#pragma unroll
            for (int i = 0; i < 8; ++i) As[(tid >> 6) + 4 * i][tid & 63] = ra[i];
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i, m = idx >> 3, kq = (idx & 7) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) As[kq + e][m] = ra[4 * i + e];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) Bs[(tid >> 6) + 4 * i][tid & 63] = rb[i];
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nk = K / 32;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        store();
        __syncthreads();
        if (kt + 1 < nk) load(kt + 1);
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * s + half][wm * 32 + c], Bs[2 * s + half][wn * 32 + c], acc, 0, 0, 0);
    }

    const int n = n0 + wn * 32 + c;
    if (n >= N) return;
    float* C = J.C + bi * J.sC;
    const float* R = J.R ? J.R + bi * J.sR : nullptr;
    float* Ct = J.Ct ? J.Ct + bi * J.sCt : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + mfma_row(r, half);
        if (m >= M) continue;
        float v = acc[r];
        if (p.scale != 1.f) v *= p.scale;
        if (J.bias) v += J.bias[m];
        if (J.bn) v = (v - J.bn[m]) / sqrtf(J.bn[J.M + m] + BN_EPS) * J.bn[2 * J.M + m] + J.bn[3 * J.M + m];
        if (p.relu) v = fmaxf(v, 0.f);
        if (R) v = R[size_t(m) * J.ldc + n] + v;
        C[size_t(m) * J.ldc + n] = v;
        if (Ct) Ct[size_t(n) * J.ldct + m] = v;
    }
}

// ---- fused softmax attention: per (side, batch, head, 128 queries); K/V tiles of 64 source points through LDS ----
// S^T = K^T Q on MFMA (rows = source, columns = queries: a lane owns one query column), online max / sum per column,
// O += V P on MFMA with P straight from the accumulator registers.  The N x M probabilities never leave registers.
struct AttnSide {
    const float* q; long sq;     // [256][N] head-contiguous
    const float* kv; long skv;   // [512][M]: k rows 0..255, v rows 256..511, head-contiguous
    float* out; long so;         // [256][N]
    int N, M;                    // capacities (leading dimensions); N == 0: a side without blocks
    int nsel, msel;              // queries / sources of an item: count(nsel), count(msel)
};
struct AttnArgs {
    AttnSide side[2];
    int b;
    Items items;
};

__global__ __launch_bounds__(256) void sg_attn_kernel(AttnArgs p) {
    const int sd = blockIdx.z / p.b, bi = blockIdx.z % p.b, hd = blockIdx.y;
    const AttnSide& S = p.side[sd];
    const int ldn = S.N, ldm = S.M, q0 = blockIdx.x * 128;
    const int N = ldn ? p.items.count(S.nsel, bi) : 0, M = p.items.count(S.msel, bi);
    if (q0 >= N) return;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, half = l >> 5, c = l & 31;
    const int myq = q0 + w * 32 + c;
    const float* Q = S.q + bi * S.sq + size_t(hd) * 64 * ldn;
    const float* Kp = S.kv + bi * S.skv + size_t(hd) * 64 * ldm;
    const float* Vp = Kp + size_t(D) * ldm;

    __shared__ float Ks[64][64];
    __shared__ float Vt[64][65];

    float qr[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) qr[s] = myq < N ? Q[size_t(2 * s + half) * ldn + myq] * 0.125f : 0.f;   // 1/sqrt(64): exact

    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float mrun = -INFINITY, lrun = 0.f;

    for (int j0 = 0; j0 < M; j0 += 64) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int src = tid & 63, d = (tid >> 6) + 4 * i;
            const bool ok = j0 + src < M;
            Ks[d][src] = ok ? Kp[size_t(d) * ldm + j0 + src] : 0.f;
            Vt[src][d] = ok ? Vp[size_t(d) * ldm + j0 + src] : 0.f;
        }
        __syncthreads();
        f32x16 s0, s1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[2 * s + half][c], qr[s], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[2 * s + half][32 + c], qr[s], s1, 0, 0, 0);
        }
        float mloc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (j0 + mfma_row(r, half) >= M) s0[r] = -INFINITY;
            if (j0 + 32 + mfma_row(r, half) >= M) s1[r] = -INFINITY;
            mloc = fmaxf(mloc, fmaxf(s0[r], s1[r]));
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float mnew = fmaxf(mrun, mloc);
        const float alpha = expf(mrun - mnew);
        float lsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = expf(s0[r] - mnew);
            s1[r] = expf(s1[r] - mnew);
            lsum += s0[r] + s1[r];
        }
        lsum += __shfl_xor(lsum, 32);
        lrun = lrun * alpha + lsum;
        mrun = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int sa = mfma_row(r, half);
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[sa][c], s0[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[sa][32 + c], s0[r], o1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int sa = 32 + mfma_row(r, half);
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[sa][c], s1[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[sa][32 + c], s1[r], o1, 0, 0, 0);
        }
    }
    if (myq >= N) return;
    const float inv = 1.f / lrun;
    float* O = S.out + bi * S.so + size_t(hd) * 64 * ldn;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        O[size_t(mfma_row(r, half)) * ldn + myq] = o0[r] * inv;
        O[size_t(32 + mfma_row(r, half)) * ldn + myq] = o1[r] * inv;
    }
}

// ---- keypoint encoder, layers 0..2 (3 -> 32 -> 64 -> 128, BatchNorm + ReLU) per point; layers 3, 4 run as GEMMs ----
struct KencSide {
    const float* kpts; const float* scores; float* h3;   // [b][N][2], [b][N], h3: [b][128][N]; N: the side's capacity
    int N;
};
struct KencNorm {
    float cx, cy, sc;                                     // normalisation: (k - c) / sc
};
struct KencArgs {
    KencSide side[2];
    const float* w;   // packed weights
    size_t w0, b0, bn0, w1, b1, bn1, w2, b2, bn2;
    int b;
    Items items;
    KencNorm norm[2][SG_MAX_ITEMS];                       // per side and item slot
};

__device__ __forceinline__ float bn_relu(float v, const float* bn, int C, int o) {
    v = (v - bn[o]) / sqrtf(bn[C + o] + BN_EPS) * bn[2 * C + o] + bn[3 * C + o];
    return fmaxf(v, 0.f);
}

__global__ __launch_bounds__(256) void sg_kenc_kernel(KencArgs p) {
    const int sd = blockIdx.z / p.b, bi = blockIdx.z % p.b;
    const KencSide& S = p.side[sd];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.items.count(sd, bi)) return;
    const KencNorm& nm = p.norm[sd][p.items.slot(bi)];
    const float* kp = S.kpts + (size_t(bi) * S.N + i) * 2;
    const float in[3] = {(kp[0] - nm.cx) / nm.sc, (kp[1] - nm.cy) / nm.sc, S.scores[size_t(bi) * S.N + i]};
    const float* W0 = p.w + p.w0; const float* B0 = p.w + p.b0; const float* N0 = p.w + p.bn0;
    const float* W1 = p.w + p.w1; const float* B1 = p.w + p.b1; const float* N1 = p.w + p.bn1;
    const float* W2 = p.w + p.w2; const float* B2 = p.w + p.b2; const float* N2 = p.w + p.bn2;
    float h1[32], h2[64];
#pragma unroll
    for (int o = 0; o < 32; ++o) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) a = fmaf(W0[o * 3 + k], in[k], a);
        h1[o] = bn_relu(a + B0[o], N0, 32, o);
    }
#pragma unroll
    for (int o = 0; o < 64; ++o) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) a = fmaf(W1[o * 32 + k], h1[k], a);
        h2[o] = bn_relu(a + B1[o], N1, 64, o);
    }
    float* out = S.h3 + size_t(bi) * 128 * S.N + i;
    for (int o = 0; o < 128; ++o) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 64; ++k) a = fmaf(W2[o * 64 + k], h2[k], a);
        out[size_t(o) * S.N] = bn_relu(a + B2[o], N2, 128, o);
    }
}

// ---- log-space Sinkhorn ----
// Coupling Z [b][cap0+1][cap1+1] and its transpose Zt [b][cap1+1][cap0+1] (bitwise the same values); item i occupies rows
// 0..n0_i and columns 0..n1_i of its slot.  Both the row update (u) and the column update (v) are contiguous row
// logsumexps: one wave per row, a fixed-order online (max, sum) per lane and a fixed butterfly across lanes.  Two launches
// per iteration.

// copy == 1: Z / Zt interior from scores [b][cap0][cap1] and the dustbins; copy == 0: dustbins only (the score GEMM wrote the
// interior).  Zeroes u and v either way (iters == 0 leaves them at zero).
__global__ void sg_sk_build_kernel(const float* scores, const float* bin, float* Z, float* Zt, float* u, float* v, int cap0, int cap1,
                                   int copy, Items T) {
    const int bi = blockIdx.y, n0 = T.count(0, bi), n1 = T.count(1, bi);
    const size_t zsz = size_t(cap0 + 1) * (cap1 + 1);
    float* z = Z + bi * zsz;
    float* zt = Zt + bi * zsz;
    const float alpha = bin[0];
    const long i = long(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i <= n0) u[size_t(bi) * (cap0 + 1) + i] = 0.f;
    if (i <= n1) v[size_t(bi) * (cap1 + 1) + i] = 0.f;
    int r, cc;
    float val = alpha;
    if (copy) {
        if (i >= long(zsz)) return;
        r = int(i / (cap1 + 1)); cc = int(i % (cap1 + 1));
        if (r > n0 || cc > n1) return;
        if (r < n0 && cc < n1) val = scores[size_t(bi) * cap0 * cap1 + size_t(r) * cap1 + cc];
    } else {
        if (i > n0 + n1) return;
        r = i < n0 ? int(i) : n0; cc = i < n0 ? n1 : int(i - n0);
    }
    z[size_t(r) * (cap1 + 1) + cc] = val;
    zt[size_t(cc) * (cap0 + 1) + r] = val;
}

__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float mn = fmaxf(m, om);
    if (mn == -INFINITY) return;
    s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + (om == -INFINITY ? 0.f : os * expf(om - mn));
    m = mn;
}

// out[row] = (row < rows - 1 ? norm : last) - logsumexp_j(Zm[row][j] + in[j]) over the item's rows x cols of a slot of
// caprows x capcols; side 0: Zm = Z (rows n0 + 1, last = mu_last), side 1: Zm = Zt (rows n1 + 1, last = nu_last)
__global__ __launch_bounds__(256) void sg_sk_rows_kernel(const float* Zm, const float* in, float* out, int side, int caprows,
                                                         int capcols, Items T, Marginals mg) {
    const int bi = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const int rows = T.count(side, bi) + 1, cols = T.count(1 - side, bi) + 1;
    if (row >= rows) return;
    const float lm = mg.norm[T.slot(bi)], lm_last = side ? mg.nu_last[T.slot(bi)] : mg.mu_last[T.slot(bi)];
    const float* z = Zm + bi * size_t(caprows) * capcols + size_t(row) * capcols;
    const float* vi = in + size_t(bi) * capcols;
    float m = -INFINITY, s = 0.f;
    for (int j = l; j < cols; j += 64) {
        const float x = z[j] + vi[j];
        if (x > m) { s = s * expf(m - x) + 1.f; m = x; }
        else s += expf(x - m);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
        lse_merge(m, s, om, os);
    }
    if (l == 0) out[size_t(bi) * caprows + row] = (row < rows - 1 ? lm : lm_last) - (m + logf(s));
}

// Zo = Z + u + v - norm (reference op order)
__global__ void sg_sk_final_kernel(const float* Z, const float* u, const float* v, float* Zo, int cap0, int cap1, Items T, Marginals mg) {
    const int bi = blockIdx.y;
    const size_t zsz = size_t(cap0 + 1) * (cap1 + 1);
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= zsz) return;
    const int r = int(i / (cap1 + 1)), cc = int(i % (cap1 + 1));
    if (r > T.count(0, bi) || cc > T.count(1, bi)) return;
    const float norm = mg.norm[T.slot(bi)];
    const float z = Z[bi * zsz + i] + u[size_t(bi) * (cap0 + 1) + r];
    Zo[bi * zsz + i] = (z + v[size_t(bi) * (cap1 + 1) + cc]) - norm;
}

// ---- match tail ----
__device__ __forceinline__ void argmax_merge(float& best, int& idx, float ob, int oi) {
    if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
}

// max / argmax of z[i][0..n1) for i < n0: one wave per row, first index wins on exact ties
__global__ __launch_bounds__(256) void sg_row_argmax_kernel(const float* Z, int cap0, int cap1, Items T, float* mx, int* ix) {
    const int bi = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const int n0 = T.count(0, bi), n1 = T.count(1, bi);
    if (row >= n0) return;
    const float* z = Z + bi * size_t(cap0 + 1) * (cap1 + 1) + size_t(row) * (cap1 + 1);
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int j = l; j < n1; j += 64) {
        const float x = z[j];
        if (x > best || idx == 0x7fffffff) { best = x; idx = j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(idx, off);
        argmax_merge(best, idx, ob, oi);
    }
    if (l == 0) { mx[size_t(bi) * cap0 + row] = best; ix[size_t(bi) * cap0 + row] = idx; }
}

// column partials over chunks of 256 rows: thread (column, quarter of 64 rows), quarters merged in row order; a chunk past
// the item's rows has no block
__global__ __launch_bounds__(256) void sg_col_partial_kernel(const float* Z, int cap0, int cap1, Items T, float* pv, int* pi) {
    const int bi = blockIdx.z, chunk = blockIdx.y, col = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const int nchunk = gridDim.y, n0 = T.count(0, bi), n1 = T.count(1, bi);
    if (chunk * 256 >= n0) return;
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    float best = -INFINITY;
    int idx = 0x7fffffff;
    if (col < n1) {
        const float* z = Z + bi * size_t(cap0 + 1) * (cap1 + 1) + col;
        const int r0 = chunk * 256 + q * 64, r1 = min(r0 + 64, n0);
        for (int r = r0; r < r1; ++r) {
            const float x = z[size_t(r) * (cap1 + 1)];
            if (x > best || idx == 0x7fffffff) { best = x; idx = r; }
        }
    }
    sv[q][threadIdx.x & 63] = best;
    si[q][threadIdx.x & 63] = idx;
    __syncthreads();
    if (q == 0 && col < n1) {
        for (int k = 1; k < 4; ++k) argmax_merge(best, idx, sv[k][threadIdx.x], si[k][threadIdx.x]);
        pv[(size_t(bi) * nchunk + chunk) * cap1 + col] = best;
        pi[(size_t(bi) * nchunk + chunk) * cap1 + col] = idx;
    }
}

// merges the item's own chunks in order; `nchunk` (of cap0) is the layout of pv / pi
__global__ void sg_col_final_kernel(const float* pv, const int* pi, int nchunk, int cap1, Items T, float* mx, int* ix) {
    const int bi = blockIdx.y, col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= T.count(1, bi)) return;
    const int mine = (T.count(0, bi) + 255) / 256;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int k = 0; k < mine; ++k)
        argmax_merge(best, idx, pv[(size_t(bi) * nchunk + k) * cap1 + col], pi[(size_t(bi) * nchunk + k) * cap1 + col]);
    mx[size_t(bi) * cap1 + col] = best;
    ix[size_t(bi) * cap1 + col] = idx;
}

__device__ __forceinline__ float mscore0(const float* mx0, const int* ix0, const int* ix1, int i) {
    return ix1[ix0[i]] == i ? expf(mx0[i]) : 0.f;
}

// mutual check, exp, threshold (reference :257-268), one thread per point of either side; -1 / 0 past an item's counts
__global__ void sg_tail_kernel(const float* mx0, const int* ix0, const int* ix1, int cap0, int cap1, Items T, float th, int64_t* m0,
                               int64_t* m1, float* s0, float* s1) {
    const int bi = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cap0 + cap1) return;
    const int n0 = T.count(0, bi), n1 = T.count(1, bi);
    const float* x0 = mx0 + size_t(bi) * cap0;
    const int* i0 = ix0 + size_t(bi) * cap0;
    const int* i1 = ix1 + size_t(bi) * cap1;
    if (k < cap0) {
        int64_t m = -1;
        float ms = 0.f;
        if (k < n0) {
            const bool mutual = i1[i0[k]] == k;
            ms = mutual ? expf(x0[k]) : 0.f;
            if (mutual && ms > th) m = i0[k];
        }
        m0[size_t(bi) * cap0 + k] = m;
        s0[size_t(bi) * cap0 + k] = ms;
    } else {
        const int j = k - cap0;
        int64_t m = -1;
        float ms = 0.f;
        if (j < n1) {
            const int i = i1[j];
            const bool mutual = i0[i] == j;
            const float ms0 = mscore0(x0, i0, i1, i);
            const bool valid0 = (i1[i0[i]] == i) && ms0 > th;
            if (mutual && valid0) m = i;
            ms = mutual ? ms0 : 0.f;
        }
        m1[size_t(bi) * cap1 + j] = m;
        s1[size_t(bi) * cap1 + j] = ms;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
struct Layout {
    int b, n0, n1, nm;       // n0 / n1: the capacities of the two sides (the counts themselves for a uniform batch)
    size_t side_floats[7];   // per-side channel counts of the activation buffers below
    size_t xa, xb, q, kv, msg, mrg, hb, z, zt, u, v, mx0, ix0, mx1, ix1, pv, pi, total;
    int nchunk;
};
enum { CH_XA = 256, CH_XB = 256, CH_Q = 256, CH_KV = 512, CH_MSG = 256, CH_MRG = 256, CH_HB = 512 };

Layout make_layout(int b, int n0, int n1) {
    Layout L{};
    L.b = b; L.n0 = n0; L.n1 = n1; L.nm = std::max(n0, n1);
    L.nchunk = (n0 + 255) / 256;
    const size_t P = size_t(b) * L.nm * 4;   // bytes per channel row-set of one side
    Bump a(nullptr);   // offsets, not pointers: the layout is built before the workspace is known
    L.xa = a.reserve(2 * CH_XA * P); L.xb = a.reserve(2 * CH_XB * P); L.q = a.reserve(2 * CH_Q * P); L.kv = a.reserve(2 * CH_KV * P);
    L.msg = a.reserve(2 * CH_MSG * P); L.mrg = a.reserve(2 * CH_MRG * P); L.hb = a.reserve(2 * CH_HB * P);
    const size_t zsz = size_t(b) * (n0 + 1) * (n1 + 1) * 4;
    L.z = a.reserve(zsz); L.zt = a.reserve(zsz);
    L.u = a.reserve(size_t(b) * (n0 + 1) * 4); L.v = a.reserve(size_t(b) * (n1 + 1) * 4);
    L.mx0 = a.reserve(size_t(b) * n0 * 4); L.ix0 = a.reserve(size_t(b) * n0 * 4);
    L.mx1 = a.reserve(size_t(b) * n1 * 4); L.ix1 = a.reserve(size_t(b) * n1 * 4);
    L.pv = a.reserve(size_t(b) * L.nchunk * n1 * 4); L.pi = a.reserve(size_t(b) * L.nchunk * n1 * 4);
    L.total = a.off;
    return L;
}

struct Ctx {
    Layout L;
    char* ws;
    hipStream_t st;
    const float* w;
    Items items;
    // side s of a per-side activation buffer with `ch` channels
    float* buf(size_t off, int ch, int s) const { return reinterpret_cast<float*>(ws + off) + size_t(s) * ch * L.b * L.nm; }
    int n(int s) const { return s ? L.n1 : L.n0; }   // capacity of side s: leading dimension and grid extent
    int slots() const { return items.uniform ? 1 : L.b; }
    float* f(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    int* i(size_t off) const { return reinterpret_cast<int*>(ws + off); }
};

Items uniform_items(int n0, int n1) {
    Items t{};
    t.uniform = 1; t.n[0][0] = n0; t.n[1][0] = n1;
    return t;
}

Ctx make_ctx(int b, int cap0, int cap1, const Items& items, void* ws, sg_stream_t stream, const float* packed) {
    return Ctx{make_layout(b, cap0, cap1), static_cast<char*>(ws), reinterpret_cast<hipStream_t>(stream), packed, items};
}

int launch_status(const char* what) { return check_launch(-3, what, ": launch failed: "); }

int check_common(int b, int n0, int n1, void* ws, size_t ws_bytes) {
    if (b < 1 || n0 < 1 || n1 < 1) return fail(-1, "b, n0, n1 must be >= 1 (got %d, %d, %d)", b, n0, n1);
    if (size_t(b) * (n0 + 1) * (n1 + 1) > (size_t(1) << 31)) return fail(-1, "problem too large");
    if (!ws) return fail(-1, "workspace is null");
    const size_t need = make_layout(b, n0, n1).total;
    if (ws_bytes < need) return fail(-2, "workspace too small: %zu bytes, need %zu", ws_bytes, need);
    return 0;
}

// the table of a ragged batch from its host arrays; everything is checked here, before any HIP call
int check_ragged(int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1, Items* items) {
    if (b < 1 || b > SG_MAX_ITEMS) return fail(-1, "b must be in [1, %d] (got %d)", SG_MAX_ITEMS, b);
    if (cap0 < 1 || cap1 < 1) return fail(-1, "cap0, cap1 must be >= 1 (got %d, %d)", cap0, cap1);
    if (!n0 || !n1) return fail(-1, "n0 / n1 (host arrays) are null");
    *items = Items{};
    for (int i = 0; i < b; ++i) {
        if (n0[i] < 1 || n0[i] > cap0) return fail(-1, "item %d: n0 = %d is outside [1, cap0 = %d]", i, n0[i], cap0);
        if (n1[i] < 1 || n1[i] > cap1) return fail(-1, "item %d: n1 = %d is outside [1, cap1 = %d]", i, n1[i], cap1);
        items->n[0][i] = n0[i]; items->n[1][i] = n1[i];
    }
    return 0;
}

GemmJob job(const float* A, const float* bias, const float* bn, const float* B, long sB, float* C, long sC, int M, int N, int nsel) {
    GemmJob j{};
    j.A = A; j.bias = bias; j.bn = bn; j.B = B; j.sB = sB; j.C = C; j.sC = sC; j.ldc = N; j.M = M; j.N = N;
    j.msel = -1; j.nsel = nsel;
    return j;
}

int gemm(const Ctx& c, GemmArgs& a, const char* what) {
    int maxm = 0, maxn = 0;
    for (int k = 0; k < a.njobs; ++k) { maxm = std::max(maxm, a.job[k].M); maxn = std::max(maxn, a.job[k].N); }
    a.b = c.L.b;
    a.items = c.items;
    if (a.scale == 0.f) a.scale = 1.f;
    if (a.ksplit == 0) a.ksplit = a.K;
    dim3 grid((maxn + 63) / 64, (maxm + 63) / 64, a.njobs * c.L.b);
    hipLaunchKernelGGL(sg_gemm_kernel, grid, dim3(256), 0, c.st, a);
    return launch_status(what);
}

float norm_scale(int h, int w) { return float(std::max(h, w)) * 0.7f; }

// hw[s]: HOST (h, w) of side s per item slot
int run_kenc(const Ctx& c, const float* const kp[2], const float* const sc[2], const float* const desc[2], const int32_t* const hw[2],
             float* const out[2]) {
    const KencOff o = kenc_offsets();
    KencArgs ka{};
    ka.w = c.w; ka.b = c.L.b; ka.items = c.items;
    ka.w0 = o.w[0]; ka.b0 = o.b[0]; ka.bn0 = o.bn[0];
    ka.w1 = o.w[1]; ka.b1 = o.b[1]; ka.bn1 = o.bn[1];
    ka.w2 = o.w[2]; ka.b2 = o.b[2]; ka.bn2 = o.bn[2];
    for (int s = 0; s < 2; ++s) {
        ka.side[s] = KencSide{kp[s], sc[s], c.buf(c.L.mrg, CH_MRG, s), c.n(s)};
        for (int i = 0; i < c.slots(); ++i) {
            const int h = hw[s][2 * i], w = hw[s][2 * i + 1];
            ka.norm[s][i] = KencNorm{float(w) / 2.f, float(h) / 2.f, norm_scale(h, w)};
        }
    }
    dim3 grid((c.L.nm + 255) / 256, 1, 2 * c.L.b);
    hipLaunchKernelGGL(sg_kenc_kernel, grid, dim3(256), 0, c.st, ka);
    if (int rc = launch_status("kenc")) return rc;
    // layer 3: 128 -> 256, BatchNorm + ReLU
    GemmArgs g3{};
    g3.njobs = 2; g3.K = 128; g3.lda = 128; g3.relu = 1;
    for (int s = 0; s < 2; ++s)
        g3.job[s] = job(c.w + o.w[3], c.w + o.b[3], c.w + o.bn[3], c.buf(c.L.mrg, CH_MRG, s), 128L * c.n(s),
                        c.buf(c.L.msg, CH_MSG, s), 256L * c.n(s), 256, c.n(s), s);
    if (int rc = gemm(c, g3, "kenc layer 3")) return rc;
    // layer 4: 256 -> 256, + descriptors
    GemmArgs g4{};
    g4.njobs = 2; g4.K = 256; g4.lda = 256;
    for (int s = 0; s < 2; ++s) {
        g4.job[s] = job(c.w + o.w[4], c.w + o.b[4], nullptr, c.buf(c.L.msg, CH_MSG, s), 256L * c.n(s), out[s], 256L * c.n(s), 256,
                        c.n(s), s);
        g4.job[s].R = desc[s]; g4.job[s].sR = 256L * c.n(s);
    }
    return gemm(c, g4, "kenc layer 4");
}

// one launch for both sides: grid (query blocks of the larger side, heads, 2 * b); blocks past an item's N return at once
int launch_attention(const AttnArgs& aa, int nmax, hipStream_t st) {
    hipLaunchKernelGGL(sg_attn_kernel, dim3((nmax + 127) / 128, SG_HEADS, 2 * aa.b), dim3(256), 0, st, aa);
    return launch_status("attention");
}

int run_layer(const Ctx& c, int layer, int kind, const float* const in[2], float* const out[2]) {
    const float* W = c.w + layer_base(layer);
    // q from x, k / v from the source (pre-update descriptors of both sides)
    GemmArgs gp{};
    gp.njobs = 4; gp.K = 256; gp.lda = 256;
    for (int s = 0; s < 2; ++s) {
        const int src = kind == SG_LAYER_CROSS ? 1 - s : s;
        gp.job[2 * s] = job(W + L_WQKV, W + L_BQKV, nullptr, in[s], 256L * c.n(s), c.buf(c.L.q, CH_Q, s), 256L * c.n(s), 256, c.n(s), s);
        gp.job[2 * s + 1] = job(W + L_WQKV + 256 * 256, W + L_BQKV + 256, nullptr, in[src], 256L * c.n(src), c.buf(c.L.kv, CH_KV, s),
                                512L * c.n(src), 512, c.n(src), src);
    }
    if (int rc = gemm(c, gp, "q/k/v projection")) return rc;
    AttnArgs aa{};
    aa.b = c.L.b; aa.items = c.items;
    for (int s = 0; s < 2; ++s) {
        const int src = kind == SG_LAYER_CROSS ? 1 - s : s;
        aa.side[s] = AttnSide{c.buf(c.L.q, CH_Q, s), 256L * c.n(s), c.buf(c.L.kv, CH_KV, s), 512L * c.n(src),
                              c.buf(c.L.msg, CH_MSG, s), 256L * c.n(s), c.n(s), c.n(src), s, src};
    }
    if (int rc = launch_attention(aa, c.L.nm, c.st)) return rc;
    GemmArgs gm{};
    gm.njobs = 2; gm.K = 256; gm.lda = 256;
    for (int s = 0; s < 2; ++s)
        gm.job[s] = job(W + L_WM, W + L_BM, nullptr, c.buf(c.L.msg, CH_MSG, s), 256L * c.n(s), c.buf(c.L.mrg, CH_MRG, s),
                        256L * c.n(s), 256, c.n(s), s);
    if (int rc = gemm(c, gm, "merge")) return rc;
    // mlp.0 on cat(x, message): split K over the two operands, BatchNorm + ReLU
    GemmArgs g0{};
    g0.njobs = 2; g0.K = 512; g0.ksplit = 256; g0.lda = 512; g0.relu = 1;
    for (int s = 0; s < 2; ++s) {
        g0.job[s] = job(W + L_W1, W + L_B1, W + L_BN1, in[s], 256L * c.n(s), c.buf(c.L.hb, CH_HB, s), 512L * c.n(s), 512, c.n(s), s);
        g0.job[s].B2 = c.buf(c.L.mrg, CH_MRG, s); g0.job[s].sB2 = 256L * c.n(s);
    }
    if (int rc = gemm(c, g0, "mlp.0")) return rc;
    // mlp.3 + residual
    GemmArgs g1{};
    g1.njobs = 2; g1.K = 512; g1.lda = 512;
    for (int s = 0; s < 2; ++s) {
        g1.job[s] = job(W + L_W2, W + L_B2, nullptr, c.buf(c.L.hb, CH_HB, s), 512L * c.n(s), out[s], 256L * c.n(s), 256, c.n(s), s);
        g1.job[s].R = in[s]; g1.job[s].sR = 256L * c.n(s);
    }
    return gemm(c, g1, "mlp.3");
}

// marginals of log_optimal_transport (:157-165), in fp32 as the reference computes them
void ot_marginals(int n0, int n1, float* norm, float* mu_last, float* nu_last) {
    const float ms = float(n0), ns = float(n1);
    *norm = -logf(ms + ns);
    *mu_last = logf(ns) + *norm;
    *nu_last = logf(ms) + *norm;
}

Marginals marginals(const Ctx& c) {
    Marginals mg{};
    for (int i = 0; i < c.slots(); ++i) ot_marginals(c.items.n[0][i], c.items.n[1][i], &mg.norm[i], &mg.mu_last[i], &mg.nu_last[i]);
    return mg;
}

// Z / Zt interior from `scores` [b][cap0][cap1] (copy) or already written by the score GEMM, plus the dustbins; u = v = 0
int run_sk_build(const Ctx& c, const float* scores, const float* bin, int copy) {
    const int cap0 = c.L.n0, cap1 = c.L.n1;
    const size_t cells = copy ? size_t(cap0 + 1) * (cap1 + 1) : size_t(std::max(cap0, cap1)) * 2 + 2;
    hipLaunchKernelGGL(sg_sk_build_kernel, dim3(unsigned((cells + 255) / 256), c.L.b), dim3(256), 0, c.st, scores, bin, c.f(c.L.z),
                       c.f(c.L.zt), c.f(c.L.u), c.f(c.L.v), cap0, cap1, copy, c.items);
    return launch_status(copy ? "sinkhorn build" : "dustbins");
}

// Z / Zt (with dustbins, u = v = 0) in the workspace -> iterations -> zo
int run_sinkhorn(const Ctx& c, int iters, float* zo) {
    const int cap0 = c.L.n0, cap1 = c.L.n1, b = c.L.b;
    const Marginals mg = marginals(c);
    float *Z = c.f(c.L.z), *Zt = c.f(c.L.zt), *u = c.f(c.L.u), *v = c.f(c.L.v);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(sg_sk_rows_kernel, dim3((cap0 + 1 + 3) / 4, b), dim3(256), 0, c.st, Z, v, u, 0, cap0 + 1, cap1 + 1, c.items, mg);
        hipLaunchKernelGGL(sg_sk_rows_kernel, dim3((cap1 + 1 + 3) / 4, b), dim3(256), 0, c.st, Zt, u, v, 1, cap1 + 1, cap0 + 1, c.items, mg);
    }
    const size_t zsz = size_t(cap0 + 1) * (cap1 + 1);
    hipLaunchKernelGGL(sg_sk_final_kernel, dim3(unsigned((zsz + 255) / 256), b), dim3(256), 0, c.st, Z, u, v, zo, cap0, cap1, c.items, mg);
    return launch_status("sinkhorn");
}

int run_tail(const Ctx& c, const float* z, float th, int64_t* m0, int64_t* m1, float* s0, float* s1) {
    const int cap0 = c.L.n0, cap1 = c.L.n1, b = c.L.b;
    hipLaunchKernelGGL(sg_row_argmax_kernel, dim3((cap0 + 3) / 4, b), dim3(256), 0, c.st, z, cap0, cap1, c.items, c.f(c.L.mx0),
                       c.i(c.L.ix0));
    hipLaunchKernelGGL(sg_col_partial_kernel, dim3((cap1 + 63) / 64, c.L.nchunk, b), dim3(256), 0, c.st, z, cap0, cap1, c.items,
                       c.f(c.L.pv), c.i(c.L.pi));
    hipLaunchKernelGGL(sg_col_final_kernel, dim3((cap1 + 255) / 256, b), dim3(256), 0, c.st, c.f(c.L.pv), c.i(c.L.pi), c.L.nchunk, cap1,
                       c.items, c.f(c.L.mx1), c.i(c.L.ix1));
    hipLaunchKernelGGL(sg_tail_kernel, dim3((cap0 + cap1 + 255) / 256, b), dim3(256), 0, c.st, c.f(c.L.mx0), c.i(c.L.ix0), c.i(c.L.ix1),
                       cap0, cap1, c.items, th, m0, m1, s0, s1);
    return launch_status("match tail");
}

int check_layers(int n_layers, const int32_t* kinds) {
    if (n_layers < 0 || n_layers > SG_MAX_LAYERS) return fail(-1, "n_layers must be in [0, %d] (got %d)", SG_MAX_LAYERS, n_layers);
    for (int l = 0; l < n_layers; ++l)
        if (!kinds || (kinds[l] != SG_LAYER_SELF && kinds[l] != SG_LAYER_CROSS))
            return fail(-1, "layer %d: kind must be SG_LAYER_SELF or SG_LAYER_CROSS", l);
    return 0;
}

int check_sizes(const Ctx& c, const int32_t* const hw[2]) {
    for (int s = 0; s < 2; ++s) {
        if (!hw[s]) return fail(-1, "hw%d (host array) is null", s);
        for (int i = 0; i < c.slots(); ++i)
            if (hw[s][2 * i] < 1 || hw[s][2 * i + 1] < 1) return fail(-1, "image sizes must be positive");
    }
    return 0;
}

// SuperGlue.forward on a checked context: the uniform and the ragged entry differ in the table alone
int run_forward(const Ctx& c, int n_layers, const int32_t* layer_kinds, int sinkhorn_iters, float match_threshold,
                const float* const kp[2], const float* const sc[2], const float* const de[2], const int32_t* const hw[2],
                int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* z_out) {
    const int cap0 = c.L.n0, cap1 = c.L.n1;
    float* xa[2] = {c.buf(c.L.xa, CH_XA, 0), c.buf(c.L.xa, CH_XA, 1)};
    float* xb[2] = {c.buf(c.L.xb, CH_XB, 0), c.buf(c.L.xb, CH_XB, 1)};
    if (int rc = run_kenc(c, kp, sc, de, hw, xa)) return rc;
    float** cur = xa;
    float** nxt = xb;
    for (int l = 0; l < n_layers; ++l) {
        const float* in[2] = {cur[0], cur[1]};
        if (int rc = run_layer(c, l, layer_kinds[l], in, nxt)) return rc;
        std::swap(cur, nxt);
    }
    // final_proj on both sides
    const float* F = c.w + final_base(n_layers);
    GemmArgs gf{};
    gf.njobs = 2; gf.K = 256; gf.lda = 256;
    for (int s = 0; s < 2; ++s)
        gf.job[s] = job(F, F + D * D, nullptr, cur[s], 256L * c.n(s), c.buf(c.L.q, CH_Q, s), 256L * c.n(s), 256, c.n(s), s);
    if (int rc = gemm(c, gf, "final_proj")) return rc;
    // scores = mdesc0^T mdesc1 / 16, written into each item's block of the coupling matrix and its transpose
    GemmArgs gs{};
    gs.njobs = 1; gs.K = 256; gs.lda = cap0; gs.a_km = 1; gs.scale = 1.f / 16.f;
    const long zsz = long(cap0 + 1) * (cap1 + 1);
    gs.job[0] = job(c.buf(c.L.q, CH_Q, 0), nullptr, nullptr, c.buf(c.L.q, CH_Q, 1), 256L * cap1, c.f(c.L.z), zsz, cap0, cap1, 1);
    gs.job[0].msel = 0;
    gs.job[0].sA = 256L * cap0;
    gs.job[0].ldc = cap1 + 1;
    gs.job[0].Ct = c.f(c.L.zt); gs.job[0].sCt = zsz; gs.job[0].ldct = cap0 + 1;
    if (int rc = gemm(c, gs, "scores")) return rc;
    if (int rc = run_sk_build(c, nullptr, c.w + OFF_BIN, 0)) return rc;
    float* zf = z_out ? z_out : c.f(c.L.z);
    if (int rc = run_sinkhorn(c, sinkhorn_iters, zf)) return rc;
    return run_tail(c, zf, match_threshold, matches0, matches1, mscores0, mscores1);
}

int run_attention(const float* q, const float* kv, int b, int capN, int capM, const Items& items, float* out, sg_stream_t stream) {
    if (size_t(b) * 2 * D * std::max(capN, capM) > (size_t(1) << 31)) return fail(-1, "problem too large");
    if (!q || !kv || !out) return fail(-1, "null argument");
    if (out == q || out == kv) return fail(-1, "out must not alias q or kv");
    // the forward's launch: side 1 has no query blocks (capacity 0 returns before any load or store)
    AttnArgs aa{};
    aa.b = b; aa.items = items;
    aa.side[0] = AttnSide{q, 256L * capN, kv, 512L * capM, out, 256L * capN, capN, capM, 0, 1};
    aa.side[1] = AttnSide{q, 256L * capN, kv, 512L * capM, out, 256L * capN, 0, capM, 0, 1};
    return launch_attention(aa, capN, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int sg_version(void) { return 3; }   // 3: the nearest-neighbour matcher (nn_matcher.h, nn_matcher.hip)
const char* sg_last_error(void) { return g_err; }

size_t sg_packed_weights_bytes(int n_layers) {
    if (n_layers < 0 || n_layers > SG_MAX_LAYERS) return 0;
    return packed_floats(n_layers) * sizeof(float);
}

int sg_pack_weights(const float* const* raw, int n_layers, float* packed, sg_stream_t stream) {
    if (n_layers < 0 || n_layers > SG_MAX_LAYERS) return fail(-1, "n_layers must be in [0, %d]", SG_MAX_LAYERS);
    if (!raw || !packed) return fail(-1, "null argument");
    for (int i = 0; i < SG_NUM_RAW(n_layers); ++i)
        if (!raw[i]) return fail(-1, "raw[%d] is null", i);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int err = 0;
    auto cp = [&](size_t dst, const float* src, int rows, int cols, int pr, int pc) {
        const int n = rows * cols;
        hipLaunchKernelGGL(sg_copy_perm_kernel, dim3((n + 255) / 256), dim3(256), 0, st, packed + dst, src, rows, cols, pr, pc);
        if (hipGetLastError() != hipSuccess) err = 1;
    };
    int r = 0;
    cp(OFF_BIN, raw[r++], 1, 1, 0, 0);
    const KencOff o = kenc_offsets();
    for (int l = 0; l < 5; ++l) {
        const int co = KENC[l + 1], ci = KENC[l];
        cp(o.w[l], raw[r++], co, ci, 0, 0);
        cp(o.b[l], raw[r++], co, 1, 0, 0);
        if (l < 4) {   // state_dict: weight (gamma), bias (beta), running_mean, running_var -> packed mean, var, gamma, beta
            const float* g = raw[r++]; const float* be = raw[r++]; const float* mu = raw[r++]; const float* var = raw[r++];
            cp(o.bn[l], mu, co, 1, 0, 0); cp(o.bn[l] + co, var, co, 1, 0, 0);
            cp(o.bn[l] + 2 * co, g, co, 1, 0, 0); cp(o.bn[l] + 3 * co, be, co, 1, 0, 0);
        }
    }
    for (int l = 0; l < n_layers; ++l) {
        const size_t B = layer_base(l);
        const float* mw = raw[r++]; const float* mb = raw[r++];
        for (int k = 0; k < 3; ++k) {   // proj.0 (q), proj.1 (k), proj.2 (v): head-contiguous rows
            cp(B + L_WQKV + size_t(k) * D * D, raw[r++], D, D, 1, 0);
            cp(B + L_BQKV + size_t(k) * D, raw[r++], D, 1, 1, 0);
        }
        cp(B + L_WM, mw, D, D, 0, 1);    // merge: head-contiguous columns
        cp(B + L_BM, mb, D, 1, 0, 0);
        cp(B + L_W1, raw[r++], 2 * D, 2 * D, 0, 0);
        cp(B + L_B1, raw[r++], 2 * D, 1, 0, 0);
        const float* g = raw[r++]; const float* be = raw[r++]; const float* mu = raw[r++]; const float* var = raw[r++];
        cp(B + L_BN1, mu, 2 * D, 1, 0, 0); cp(B + L_BN1 + 2 * D, var, 2 * D, 1, 0, 0);
        cp(B + L_BN1 + 4 * D, g, 2 * D, 1, 0, 0); cp(B + L_BN1 + 6 * D, be, 2 * D, 1, 0, 0);
        cp(B + L_W2, raw[r++], D, 2 * D, 0, 0);
        cp(B + L_B2, raw[r++], D, 1, 0, 0);
    }
    cp(final_base(n_layers), raw[r++], D, D, 0, 0);
    cp(final_base(n_layers) + D * D, raw[r++], D, 1, 0, 0);
    if (err) return fail(-3, "sg_pack_weights: launch failed");
    return 0;
}

size_t sg_workspace_bytes(int b, int n0, int n1) {
    if (b < 1 || n0 < 1 || n1 < 1) return 0;
    return make_layout(b, n0, n1).total;
}

size_t sg_ragged_workspace_bytes(int b, int cap0, int cap1) {
    if (b > SG_MAX_ITEMS) return 0;
    return sg_workspace_bytes(b, cap0, cap1);
}

int sg_keypoint_encode(const float* packed, int n_layers, const float* kpts0, const float* scores0, const float* desc0,
                       const float* kpts1, const float* scores1, const float* desc1, int b, int n0, int n1, int h0, int w0, int h1,
                       int w1, float* out0, float* out1, void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    if (int rc = check_common(b, n0, n1, workspace, workspace_bytes)) return rc;
    if (!packed || !kpts0 || !scores0 || !desc0 || !kpts1 || !scores1 || !desc1 || !out0 || !out1) return fail(-1, "null argument");
    if (h0 < 1 || w0 < 1 || h1 < 1 || w1 < 1) return fail(-1, "image sizes must be positive");
    (void)n_layers;
    const Ctx c = make_ctx(b, n0, n1, uniform_items(n0, n1), workspace, stream, packed);
    const float* kp[2] = {kpts0, kpts1};
    const float* sc[2] = {scores0, scores1};
    const float* de[2] = {desc0, desc1};
    const int32_t hw0[2] = {h0, w0}, hw1[2] = {h1, w1};
    const int32_t* hw[2] = {hw0, hw1};
    float* out[2] = {out0, out1};
    return run_kenc(c, kp, sc, de, hw, out);
}

int sg_layer(const float* packed, int n_layers, int layer, int kind, const float* desc0, const float* desc1, int b, int n0, int n1,
             float* out0, float* out1, void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    if (int rc = check_common(b, n0, n1, workspace, workspace_bytes)) return rc;
    if (!packed || !desc0 || !desc1 || !out0 || !out1) return fail(-1, "null argument");
    if (layer < 0 || layer >= n_layers || n_layers > SG_MAX_LAYERS) return fail(-1, "layer %d out of range [0, %d)", layer, n_layers);
    if (kind != SG_LAYER_SELF && kind != SG_LAYER_CROSS) return fail(-1, "kind must be SG_LAYER_SELF or SG_LAYER_CROSS");
    if (out0 == desc0 || out0 == desc1 || out1 == desc0 || out1 == desc1) return fail(-1, "outputs must not alias the inputs");
    const Ctx c = make_ctx(b, n0, n1, uniform_items(n0, n1), workspace, stream, packed);
    const float* in[2] = {desc0, desc1};
    float* out[2] = {out0, out1};
    return run_layer(c, layer, kind, in, out);
}

int sg_attention(const float* q, const float* kv, int b, int N, int M, float* out, sg_stream_t stream) {
    if (b < 1 || N < 1 || M < 1) return fail(-1, "b, N, M must be >= 1 (got %d, %d, %d)", b, N, M);
    return run_attention(q, kv, b, N, M, uniform_items(N, M), out, stream);
}

int sg_attention_ragged(const float* q, const float* kv, int b, int capN, int capM, const int32_t* n, const int32_t* m, float* out,
                        sg_stream_t stream) {
    Items items;
    if (int rc = check_ragged(b, capN, capM, n, m, &items)) return rc;
    return run_attention(q, kv, b, capN, capM, items, out, stream);
}

int sg_sinkhorn(const float* scores, const float* bin_score, int b, int n0, int n1, int iters, float* z_out, void* workspace,
                size_t workspace_bytes, sg_stream_t stream) {
    if (int rc = check_common(b, n0, n1, workspace, workspace_bytes)) return rc;
    if (!scores || !bin_score || !z_out) return fail(-1, "null argument");
    if (iters < 0) return fail(-1, "iters must be >= 0");
    const Ctx c = make_ctx(b, n0, n1, uniform_items(n0, n1), workspace, stream, nullptr);
    if (int rc = run_sk_build(c, scores, bin_score, 1)) return rc;
    return run_sinkhorn(c, iters, z_out);
}

int sg_sinkhorn_ragged(const float* scores, const float* bin_score, int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1,
                       int iters, float* z_out, void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    Items items;
    if (int rc = check_ragged(b, cap0, cap1, n0, n1, &items)) return rc;
    if (int rc = check_common(b, cap0, cap1, workspace, workspace_bytes)) return rc;
    if (!scores || !bin_score || !z_out) return fail(-1, "null argument");
    if (iters < 0) return fail(-1, "iters must be >= 0");
    const Ctx c = make_ctx(b, cap0, cap1, items, workspace, stream, nullptr);
    if (int rc = run_sk_build(c, scores, bin_score, 1)) return rc;
    return run_sinkhorn(c, iters, z_out);
}

int sg_match_tail(const float* z, int b, int n0, int n1, float match_threshold, int64_t* matches0, int64_t* matches1,
                  float* mscores0, float* mscores1, void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    if (int rc = check_common(b, n0, n1, workspace, workspace_bytes)) return rc;
    if (!z || !matches0 || !matches1 || !mscores0 || !mscores1) return fail(-1, "null argument");
    const Ctx c = make_ctx(b, n0, n1, uniform_items(n0, n1), workspace, stream, nullptr);
    return run_tail(c, z, match_threshold, matches0, matches1, mscores0, mscores1);
}

int sg_match_tail_ragged(const float* z, int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1, float match_threshold,
                         int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, void* workspace,
                         size_t workspace_bytes, sg_stream_t stream) {
    Items items;
    if (int rc = check_ragged(b, cap0, cap1, n0, n1, &items)) return rc;
    if (int rc = check_common(b, cap0, cap1, workspace, workspace_bytes)) return rc;
    if (!z || !matches0 || !matches1 || !mscores0 || !mscores1) return fail(-1, "null argument");
    const Ctx c = make_ctx(b, cap0, cap1, items, workspace, stream, nullptr);
    return run_tail(c, z, match_threshold, matches0, matches1, mscores0, mscores1);
}

int sg_forward(const float* packed, int n_layers, const int32_t* layer_kinds, int sinkhorn_iters, float match_threshold,
               const float* kpts0, const float* scores0, const float* desc0, const float* kpts1, const float* scores1,
               const float* desc1, int b, int n0, int n1, int h0, int w0, int h1, int w1, int64_t* matches0, int64_t* matches1,
               float* mscores0, float* mscores1, float* z_out, void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    if (int rc = check_common(b, n0, n1, workspace, workspace_bytes)) return rc;
    if (int rc = check_layers(n_layers, layer_kinds)) return rc;
    if (sinkhorn_iters < 0) return fail(-1, "sinkhorn_iters must be >= 0");
    if (!packed || !kpts0 || !scores0 || !desc0 || !kpts1 || !scores1 || !desc1 || !matches0 || !matches1 || !mscores0 || !mscores1)
        return fail(-1, "null argument");
    if (h0 < 1 || w0 < 1 || h1 < 1 || w1 < 1) return fail(-1, "image sizes must be positive");
    const Ctx c = make_ctx(b, n0, n1, uniform_items(n0, n1), workspace, stream, packed);
    const float* kp[2] = {kpts0, kpts1};
    const float* sc[2] = {scores0, scores1};
    const float* de[2] = {desc0, desc1};
    const int32_t hw0[2] = {h0, w0}, hw1[2] = {h1, w1};
    const int32_t* hw[2] = {hw0, hw1};
    return run_forward(c, n_layers, layer_kinds, sinkhorn_iters, match_threshold, kp, sc, de, hw, matches0, matches1, mscores0,
                       mscores1, z_out);
}

int sg_forward_ragged(const float* packed, int n_layers, const int32_t* layer_kinds, int sinkhorn_iters, float match_threshold,
                      const float* kpts0, const float* scores0, const float* desc0, const float* kpts1, const float* scores1,
                      const float* desc1, int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1, const int32_t* hw0,
                      const int32_t* hw1, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* z_out,
                      void* workspace, size_t workspace_bytes, sg_stream_t stream) {
    Items items;
    if (int rc = check_ragged(b, cap0, cap1, n0, n1, &items)) return rc;
    if (int rc = check_common(b, cap0, cap1, workspace, workspace_bytes)) return rc;
    if (int rc = check_layers(n_layers, layer_kinds)) return rc;
    if (sinkhorn_iters < 0) return fail(-1, "sinkhorn_iters must be >= 0");
    if (!packed || !kpts0 || !scores0 || !desc0 || !kpts1 || !scores1 || !desc1 || !matches0 || !matches1 || !mscores0 || !mscores1)
        return fail(-1, "null argument");
    const Ctx c = make_ctx(b, cap0, cap1, items, workspace, stream, packed);
    const int32_t* hw[2] = {hw0, hw1};
    if (int rc = check_sizes(c, hw)) return rc;
    const float* kp[2] = {kpts0, kpts1};
    const float* sc[2] = {scores0, scores1};
    const float* de[2] = {desc0, desc1};
    return run_forward(c, n_layers, layer_kinds, sinkhorn_iters, match_threshold, kp, sc, de, hw, matches0, matches1, mscores0,
                       mscores1, z_out);
}

}  // extern "C"
