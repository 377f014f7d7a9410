// Training head of the GATsSPG matcher on gfx950 (include/gatsspg_train.h): score contraction, dual softmax and focal loss over
// the b x n x m matrix, with the analytic backward.  fp32 throughout: the three contractions run on v_mfma_f32_32x32x2_f32
// through the main loop of gemm_f32_mfma.h, everything else on fp32 VALU; the loss combine is fp64.
//
// Launches of gtr_loss_head (the header states the mathematics):
//   gtr_pack_kernel         x [256][n], y [256][m] -> planes [256][ldn], [256][ldm], zero-filled to the tile;
//   gtr_pack_t_kernel       y -> [ldm][256] (the B operand of the dx contraction), zero rows past m;
//   gtr_score_exp_kernel    one workgroup per 128 x 64 tile of x^T y: E = exp(. / s) written ONCE, zeros in the padding, and the
//                           tile's row and column sums as partials [row][column tile], [column][row tile];
//   gtr_rc_kernel           r, c: the partials in ascending tile order;
//   gtr_terms_kernel        one workgroup per tile, streaming E and the classes: loss sums and counts per tile, rowsum / colsum
//                           partials of H, positives and negatives apart (their weights need the batch's counts);
//   gtr_loss_final_kernel   one workgroup: the per-tile sums in fp64 (wg::tree_sum), the loss, the counts;
//   gtr_hsum_kernel         rowsum(H), colsum(H) from the partials and the weights;
//   gtr_ds_kernel           E <- dS in place, zeros in the padding (the K padding of the two contractions below);
//   gtr_grad_gemm_kernel    dx^T = dS y^T / s (A = dS row-major, K = ldm) and dy = x dS / s (A = the x plane, K = ldn).
// Every reduction runs in a fixed order that depends on the shape alone (no atomics): two calls are bitwise identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/gatsspg_train.h"
#include "capi_common.h"
#include "gemm_f32_mfma.h"
#include "wg_primitives.h"

namespace {

using namespace capi;
using gatsspg::f32x16;
using gatsspg::vf4;

constexpr int D = GTR_DESC_DIM;
constexpr int BM = 128, BN = 64;
using STile = gatsspg::GemmTile<BM, BN, 4, 2, true>;     // score: A = the x plane, K-major (as nn_matcher.hip)
using GTile = gatsspg::GemmTile<BM, BN, 4, 2, false>;    // gradients: A row-major (dS, or the x plane read along n)
constexpr int TS = BN + 1;                               // row stride of the staged tile: conflict-free column walks
constexpr int COLPART_OFF = BM * TS;                     // [8][BN] column part sums behind the staged tile
constexpr int PT = 256;                                  // threads of the streaming passes: 16 x 16, four columns a thread
static_assert(COLPART_OFF + STile::THREADS <= STile::SMEM_FLOATS && BM * TS <= GTile::SMEM_FLOATS, "the staged tile must fit the operand buffers");
static_assert(D % (2 * gatsspg::BK) == 0 && D % BN == 0 && D % BM == 0, "whole slabs and tiles over the channels");

struct Layout {
    int b, n, m, ldn, ldm, nrt, nct;
    size_t tiles;                                                     // nrt * nct
    size_t px, py, pyt, e, rowpart, colpart, r, c, hrow, hcol, rowh, colh, lsum, lcnt, total;   // byte offsets
};

Layout make_layout(int b, int n, int m) {
    Layout L{};
    L.b = b; L.n = n; L.m = m;
    L.ldn = round_up(n, BM); L.ldm = round_up(m, BN);
    L.nrt = L.ldn / BM; L.nct = L.ldm / BN;
    L.tiles = size_t(L.nrt) * L.nct;
    Bump a(nullptr);
    const size_t B = size_t(b);
    L.px = a.reserve(sizeof(float) * B * D * L.ldn);
    L.py = a.reserve(sizeof(float) * B * D * L.ldm);
    L.pyt = a.reserve(sizeof(float) * B * L.ldm * D);
    L.e = a.reserve(sizeof(float) * B * L.ldn * L.ldm);
    L.rowpart = a.reserve(sizeof(float) * B * L.ldn * L.nct);        // [item][row][column tile]
    L.colpart = a.reserve(sizeof(float) * B * L.ldm * L.nrt);        // [item][column][row tile]
    L.r = a.reserve(sizeof(float) * B * L.ldn);
    L.c = a.reserve(sizeof(float) * B * L.ldm);
    L.hrow = a.reserve(sizeof(float2) * B * L.ldn * L.nct);          // {positives, negatives}
    L.hcol = a.reserve(sizeof(float2) * B * L.ldm * L.nrt);
    L.rowh = a.reserve(sizeof(float) * B * L.ldn);
    L.colh = a.reserve(sizeof(float) * B * L.ldm);
    L.lsum = a.reserve(sizeof(float2) * B * L.tiles);                // per tile: sum of l over its positives, its negatives
    L.lcnt = a.reserve(sizeof(int4) * B * L.tiles);                  // per tile: positives, negatives, ignored
    L.total = a.off;
    return L;
}

// ---- pack (as nnm_pack_kernel): plane z < b is x of item z, plane b + i is y of item i ----
__global__ __launch_bounds__(256) void gtr_pack_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ PX,
                                                       float* __restrict__ PY, int b, int n, int m, int ldn, int ldm) {
    const int z = blockIdx.z, k = blockIdx.y, side = z >= b, item = side ? z - b : z;
    const int cnt = side ? m : n, ld = side ? ldm : ldn;
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= ld) return;
    const float* src = (side ? y : x) + (size_t(item) * D + k) * cnt;
    vf4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c + j < cnt ? src[c + j] : 0.f;
    *reinterpret_cast<vf4*>((side ? PY : PX) + (size_t(item) * D + k) * ld + c) = v;
}

// y [256][m] -> [ldm][256] through a 64 x 64 LDS tile; grid (ldm / 64, 256 / 64, b)
__global__ __launch_bounds__(256) void gtr_pack_t_kernel(const float* __restrict__ y, float* __restrict__ PYT, int m, int ldm) {
    __shared__ float tile[64][65];
    const int item = blockIdx.z, kb = blockIdx.y * 64, jb = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int kk = ty + 4 * q, j = jb + tx;
        tile[kk][tx] = j < m ? y[(size_t(item) * D + kb + kk) * m + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int jj = ty + 4 * q;                                    // jb + jj < ldm: the grid covers ldm exactly
        PYT[(size_t(item) * ldm + jb + jj) * D + kb + tx] = tile[tx][jj];
    }
}

// ---- score tile + exp + row / column sum partials ----
struct ScoreArgs {
    const float *PX, *PY;
    float* E;
    float *rowpart, *colpart;
    int n, m, ldn, ldm, nrt, nct;
    float scale;
};

__global__ __launch_bounds__(STile::THREADS) void gtr_score_exp_kernel(ScoreArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int rt, ct;
    if (!gatsspg::xcd_tile_map(p.nrt, p.nct, rt, ct)) return;
    const int item = blockIdx.y, ldn = p.ldn, ldm = p.ldm;
    const float* Ap = p.PX + size_t(item) * D * ldn + rt * BM;       // K-major A: [256][ldn], the tile's 128 points contiguous
    const float* Bp = p.PY + size_t(item) * D * ldm + ct * BN;
    f32x16 acc[STile::TM][STile::TN];
    gatsspg::zero_acc(acc);
    gatsspg::gemm_mainloop<STile>(
        acc, smem, D / gatsspg::BK, [&](int kt) { return Ap + size_t(kt) * gatsspg::BK * ldn; }, ldn,
        [&](int kt) { return Bp + size_t(kt) * gatsspg::BK * ldm; }, ldm);

    // the accumulators leave through LDS (the main loop ends on a barrier): staged tile [128][65]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / STile::WN, wn = wave % STile::WN, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) smem[(wm * 32 + gatsspg::mfma_row(r, half)) * TS + wn * 32 + l31] = acc[0][0][r];
    __syncthreads();
    const int rows = min(BM, p.n - rt * BM), cols = min(BN, p.m - ct * BN);   // the tile's valid extent
    float* Et = p.E + (size_t(item) * ldn + size_t(rt) * BM) * ldm + ct * BN;
    for (int idx = tid; idx < BM * BN; idx += STile::THREADS) {       // a wave writes one 256-byte row segment; padding <- 0
        const int row = idx / BN, col = idx % BN;
        const float e = row < rows && col < cols ? expf(smem[row * TS + col] / p.scale) : 0.f;
        smem[row * TS + col] = e;
        Et[size_t(row) * ldm + col] = e;
    }
    __syncthreads();
    // rows: four lanes per row, 16 consecutive columns each in column order, then the four in a fixed tree
    {
        constexpr int LPR = STile::THREADS / BM, CPL = BN / LPR;
        const int row = tid / LPR, hp = tid % LPR;
        const float* tr = smem + row * TS + hp * CPL;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) s += tr[k];
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
        if (hp == 0) p.rowpart[(size_t(item) * ldn + rt * BM + row) * p.nct + ct] = s;
    }
    // columns: eight groups of 16 rows, one thread per (group, column), then the groups in row order
    {
        constexpr int NQ = STile::THREADS / BN, RPQ = BM / NQ;
        const int c = tid % BN, q = tid / BN;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < RPQ; ++k) s += smem[(q * RPQ + k) * TS + c];
        float* part = smem + COLPART_OFF;
        part[q * BN + c] = s;
        __syncthreads();
        if (tid < BN) {
            float a = 0.f;
#pragma unroll
            for (int g = 0; g < NQ; ++g) a += part[g * BN + tid];
            p.colpart[(size_t(item) * ldm + ct * BN + tid) * p.nrt + rt] = a;
        }
    }
}

// r [item][i] (stride ldr), c [item][j] (stride ldc): the partials in ascending tile order; grid (ceil((n + m) / 256), b)
__global__ __launch_bounds__(256) void gtr_rc_kernel(const float* __restrict__ rowpart, const float* __restrict__ colpart, int n, int m,
                                                     int ldn, int ldm, int nrt, int nct, float* __restrict__ r, int ldr,
                                                     float* __restrict__ c, int ldc) {
    const int item = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n + m) return;
    if (k < n) {
        const float* part = rowpart + (size_t(item) * ldn + k) * nct;
        float s = 0.f;
        for (int t = 0; t < nct; ++t) s += part[t];
        r[size_t(item) * ldr + k] = s;
    } else {
        const int j = k - n;
        const float* part = colpart + (size_t(item) * ldm + j) * nrt;
        float s = 0.f;
        for (int t = 0; t < nrt; ++t) s += part[t];
        c[size_t(item) * ldc + j] = s;
    }
}

// ---- the focal term of one entry: l, and h = dl/dC * C (H before the weight of its class) ----
struct Focal {
    float alpha, gamma;
    int g2;                           // gamma == 2: products, as torch.pow(., 2)
};
__device__ __forceinline__ float powg(float x, float e) { return e == 0.f ? 1.f : exp2f(e * log2f(x)); }
__device__ __forceinline__ void focal_term(bool positive, float C, const Focal& f, float& l, float& h) {
    const float omc = 1.f - C;
    if (positive) {
        const float lnC = logf(C);
        const float pg = f.g2 ? omc * omc : powg(omc, f.gamma);
        const float pg1 = f.g2 ? omc : powg(omc, f.gamma - 1.f);
        l = -f.alpha * pg * lnC;
        const float t = lnC == 0.f ? 0.f : f.gamma * pg1 * C * lnC;   // C == 1: 0, whatever (1 - C)^(gamma - 1) is
        h = f.alpha * (t - pg);
    } else {
        const float l1m = logf(omc);                                   // the reference's log(1 - C) in fp32
        const float qg = f.g2 ? C * C : powg(C, f.gamma);
        l = -(1.f - f.alpha) * qg * l1m;
        h = (1.f - f.alpha) * qg * (C / omc - f.gamma * l1m);
    }
}

// What the two streaming passes read.  E is the padded matrix of the workspace; r, c and the H sums have the caller's strides.
struct PassArgs {
    float* E;                         // [item][ldn][ldm]
    const float *r, *c;               // [item][ldr], [item][ldc]
    const float *rowh, *colh;         // strides ldr, ldc (gtr_ds_kernel)
    const int8_t* cls;                // [item][n][m]
    const int64_t* counts;            // [3] (gtr_ds_kernel, gtr_hsum_kernel)
    int n, m, ldn, ldm, nrt, nct, ldr, ldc;
    int cls4;                         // rows of cls are 4-byte aligned: one load per four classes
    Focal f;
    float pos_w, neg_w;
};

// the classes of four consecutive columns (columns >= m: ignored)
__device__ __forceinline__ void load_classes(const PassArgs& p, const int8_t* row, int col0, int (&k)[4]) {
    if (p.cls4) {
        const int w = col0 < p.m ? *reinterpret_cast<const int*>(row + col0) : 0x02020202;
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = int(int8_t(w >> (8 * q)));
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = col0 + q < p.m ? int(row[col0 + q]) : GTR_CLASS_IGNORED;
    }
}

__device__ __forceinline__ void class_weights(const PassArgs& p, float& wp, float& wn) {
    const int64_t np = p.counts[0], nn = p.counts[1];
    wp = np > 0 ? float(double(p.pos_w) / double(np)) : 0.f;
    wn = nn > 0 ? float(double(p.neg_w) / double(nn)) : 0.f;
}

// One workgroup per 128 x 64 tile (blockIdx.x = rt * nct + ct), 16 x 16 threads, a thread four columns of eight rows.
__global__ __launch_bounds__(PT) void gtr_terms_kernel(PassArgs p, float2* __restrict__ hrow, float2* __restrict__ hcol,
                                                       float2* __restrict__ lsum, int4* __restrict__ lcnt) {
    __shared__ float2 colred[16][BN];
    __shared__ float wsum[PT / 64][2];
    __shared__ int wcnt[PT / 64][3];
    const int item = blockIdx.y, rt = blockIdx.x / p.nct, ct = blockIdx.x % p.nct;
    const int t = threadIdx.x, lx = t & 15, ly = t >> 4;
    const int col0 = ct * BN + lx * 4;
    float cj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cj[q] = col0 + q < p.m ? p.c[size_t(item) * p.ldc + col0 + q] : 1.f;
    float cp[4] = {0.f, 0.f, 0.f, 0.f}, cn[4] = {0.f, 0.f, 0.f, 0.f};
    float lp = 0.f, ln = 0.f;
    int np = 0, nn = 0, ni = 0;
    for (int rr = 0; rr < BM / 16; ++rr) {
        const int row = rt * BM + ly + 16 * rr;
        float rp = 0.f, rn = 0.f;
        if (row < p.n) {
            const vf4 e = gatsspg::ldg4(p.E + (size_t(item) * p.ldn + row) * p.ldm + col0);
            const float ri = p.r[size_t(item) * p.ldr + row];
            int k[4];
            load_classes(p, p.cls + (size_t(item) * p.n + row) * p.m, col0, k);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (col0 + q >= p.m) continue;
                if (k[q] != GTR_CLASS_POSITIVE && k[q] != GTR_CLASS_NEGATIVE) { ++ni; continue; }
                const float C = (e[q] / cj[q]) * (e[q] / ri);
                float l, h;
                focal_term(k[q] == GTR_CLASS_POSITIVE, C, p.f, l, h);
                if (k[q] == GTR_CLASS_POSITIVE) { lp += l; ++np; cp[q] += h; rp += h; }
                else { ln += l; ++nn; cn[q] += h; rn += h; }
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { rp += __shfl_xor(rp, o); rn += __shfl_xor(rn, o); }
        if (lx == 0) hrow[(size_t(item) * p.ldn + row) * p.nct + ct] = make_float2(rp, rn);   // row < ldn: padding rows get zeros
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) colred[ly][lx * 4 + q] = make_float2(cp[q], cn[q]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        lp += __shfl_xor(lp, o); ln += __shfl_xor(ln, o);
        np += __shfl_xor(np, o); nn += __shfl_xor(nn, o); ni += __shfl_xor(ni, o);
    }
    if ((t & 63) == 0) {
        wsum[t >> 6][0] = lp; wsum[t >> 6][1] = ln;
        wcnt[t >> 6][0] = np; wcnt[t >> 6][1] = nn; wcnt[t >> 6][2] = ni;
    }
    __syncthreads();
    if (t < BN) {
        float2 s = make_float2(0.f, 0.f);
#pragma unroll
        for (int g = 0; g < 16; ++g) { s.x += colred[g][t].x; s.y += colred[g][t].y; }
        hcol[(size_t(item) * p.ldm + ct * BN + t) * p.nrt + rt] = s;
    }
    if (t == 0) {
        float2 s = make_float2(0.f, 0.f);
        int4 c = make_int4(0, 0, 0, 0);
        for (int w = 0; w < PT / 64; ++w) { s.x += wsum[w][0]; s.y += wsum[w][1]; c.x += wcnt[w][0]; c.y += wcnt[w][1]; c.z += wcnt[w][2]; }
        const size_t tile = size_t(item) * gridDim.x + blockIdx.x;
        lsum[tile] = s;
        lcnt[tile] = c;
    }
}

// One workgroup: the per-tile sums in fp64, thread t the tiles t, t + 256, .. in ascending order, then wg::tree_sum.
__global__ __launch_bounds__(256) void gtr_loss_final_kernel(const float2* __restrict__ lsum, const int4* __restrict__ lcnt, size_t tiles,
                                                             double pos_w, double neg_w, double* __restrict__ loss_sums,
                                                             int64_t* __restrict__ counts, float* __restrict__ loss) {
    __shared__ double red[5 * 256];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t i = threadIdx.x; i < tiles; i += 256) {
        const float2 s = lsum[i];
        const int4 c = lcnt[i];
        v[0] += double(s.x); v[1] += double(s.y);
        v[2] += double(c.x); v[3] += double(c.y); v[4] += double(c.z);   // counts: integers below 2^53, exact
    }
    wg::tree_sum<256, 5>(v, red);
    if (threadIdx.x == 0) {
        double l = 0.0;
        if (v[2] > 0.0) l += pos_w * (v[0] / v[2]);
        if (v[3] > 0.0) l += neg_w * (v[1] / v[3]);
        loss[0] = float(l);
        counts[0] = int64_t(v[2]); counts[1] = int64_t(v[3]); counts[2] = int64_t(v[4]);
        if (loss_sums) { loss_sums[0] = v[0]; loss_sums[1] = v[1]; }
    }
}

// rowsum(H) [item][i], colsum(H) [item][j]: the positive and the negative partials each in ascending tile order, then weighted
__global__ __launch_bounds__(256) void gtr_hsum_kernel(PassArgs p, const float2* __restrict__ hrow, const float2* __restrict__ hcol,
                                                       float* __restrict__ rowh, float* __restrict__ colh) {
    const int item = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= p.n + p.m) return;
    float wp, wn;
    class_weights(p, wp, wn);
    const bool isrow = k < p.n;
    const int j = isrow ? k : k - p.n, cnt = isrow ? p.nct : p.nrt;
    const float2* part = isrow ? hrow + (size_t(item) * p.ldn + j) * p.nct : hcol + (size_t(item) * p.ldm + j) * p.nrt;
    float sp = 0.f, sn = 0.f;
    for (int t = 0; t < cnt; ++t) { sp += part[t].x; sn += part[t].y; }
    const float s = wp * sp + wn * sn;
    if (isrow) rowh[size_t(item) * p.ldr + j] = s;
    else colh[size_t(item) * p.ldc + j] = s;
}

// E <- dS = 2 H - A colsum_j(H) - B rowsum_i(H) in place, zeros in the padding; the geometry of gtr_terms_kernel
__global__ __launch_bounds__(PT) void gtr_ds_kernel(PassArgs p) {
    const int item = blockIdx.y, rt = blockIdx.x / p.nct, ct = blockIdx.x % p.nct;
    const int t = threadIdx.x, lx = t & 15, ly = t >> 4;
    const int col0 = ct * BN + lx * 4;
    float wp, wn;
    class_weights(p, wp, wn);
    float cj[4], chj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = col0 + q < p.m;
        cj[q] = in ? p.c[size_t(item) * p.ldc + col0 + q] : 1.f;
        chj[q] = in ? p.colh[size_t(item) * p.ldc + col0 + q] : 0.f;
    }
    for (int rr = 0; rr < BM / 16; ++rr) {
        const int row = rt * BM + ly + 16 * rr;                       // < ldn
        float* ep = p.E + (size_t(item) * p.ldn + row) * p.ldm + col0;
        vf4 out = {0.f, 0.f, 0.f, 0.f};
        if (row < p.n) {
            const vf4 e = gatsspg::ldg4(ep);
            const float ri = p.r[size_t(item) * p.ldr + row], rhi = p.rowh[size_t(item) * p.ldr + row];
            int k[4];
            load_classes(p, p.cls + (size_t(item) * p.n + row) * p.m, col0, k);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (col0 + q >= p.m) continue;
                const float A = e[q] / cj[q], B = e[q] / ri;
                float H = 0.f;
                if (k[q] == GTR_CLASS_POSITIVE || k[q] == GTR_CLASS_NEGATIVE) {
                    float l, h;
                    focal_term(k[q] == GTR_CLASS_POSITIVE, A * B, p.f, l, h);
                    H = (k[q] == GTR_CLASS_POSITIVE ? wp : wn) * h;
                }
                out[q] = 2.f * H - A * chj[q] - B * rhi;
            }
        }
        *reinterpret_cast<vf4*>(ep) = out;
    }
}

// ---- the two gradient contractions.  DX: tile rows = points i, tile columns = channels; out dx [item][256][n].
//      else: tile rows = channels, tile columns = points j; out dy [item][256][m]. ----
struct GradArgs {
    const float *A, *B;
    size_t a_item, b_item;            // item strides in floats
    int lda, ldb, KT, nrt, nct;
    float* out;
    int cnt;                          // n (DX) or m
    float inv_s;
};

template <bool DX>
__global__ __launch_bounds__(GTile::THREADS) void gtr_grad_gemm_kernel(GradArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int rt, ct;
    if (!gatsspg::xcd_tile_map(p.nrt, p.nct, rt, ct)) return;
    const int item = blockIdx.y, lda = p.lda, ldb = p.ldb;
    const float* Ap = p.A + item * p.a_item + size_t(rt) * BM * lda;
    const float* Bp = p.B + item * p.b_item + ct * BN;
    f32x16 acc[GTile::TM][GTile::TN];
    gatsspg::zero_acc(acc);
    gatsspg::gemm_mainloop<GTile>(
        acc, smem, p.KT, [&](int kt) { return Ap + size_t(kt) * gatsspg::BK; }, lda,
        [&](int kt) { return Bp + size_t(kt) * gatsspg::BK * ldb; }, ldb);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / GTile::WN, wn = wave % GTile::WN, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) smem[(wm * 32 + gatsspg::mfma_row(r, half)) * TS + wn * 32 + l31] = acc[0][0][r];
    __syncthreads();
    if constexpr (DX) {
        const int rows = min(BM, p.cnt - rt * BM);
        float* o = p.out + (size_t(item) * D + ct * BN) * p.cnt + rt * BM;
        for (int idx = tid; idx < BM * BN; idx += GTile::THREADS) {   // transposed: a wave writes 64 consecutive points of one channel
            const int col = idx / BM, row = idx % BM;
            if (row < rows) o[size_t(col) * p.cnt + row] = smem[row * TS + col] * p.inv_s;
        }
    } else {
        const int cols = min(BN, p.cnt - ct * BN);
        float* o = p.out + (size_t(item) * D + rt * BM) * p.cnt + ct * BN;
        for (int idx = tid; idx < BM * BN; idx += GTile::THREADS) {
            const int row = idx / BN, col = idx % BN;
            if (col < cols) o[size_t(row) * p.cnt + col] = smem[row * TS + col] * p.inv_s;
        }
    }
}

// dense [item][rows][cols] <-> padded [item][..][ld] (the stage entry points); grid (ceil(rows * cols / 256), b)
__global__ __launch_bounds__(256) void gtr_copy_kernel(const float* __restrict__ src, size_t s_item, int s_ld, float* __restrict__ dst,
                                                       size_t d_item, int d_ld, int rows, int cols) {
    const size_t idx = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= size_t(rows) * cols) return;
    const size_t row = idx / cols, col = idx % cols;
    dst[blockIdx.y * d_item + row * d_ld + col] = src[blockIdx.y * s_item + row * s_ld + col];
}

// ---- gtr_build_target ----
struct TargetItems {
    int k[GTR_MAX_BATCH], n_orig[GTR_MAX_BATCH], m_orig[GTR_MAX_BATCH];
};

// every entry <- negative, or the pad class in the rows >= n_orig and the columns >= m_orig; grid (ceil(n * m / 256), b)
__global__ __launch_bounds__(256) void gtr_target_fill_kernel(int8_t* __restrict__ cls, int n, int m, int pad_class, TargetItems T) {
    const size_t idx = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= size_t(n) * m) return;
    const int item = blockIdx.y, i = int(idx / m), j = int(idx % m);
    cls[size_t(item) * n * m + idx] = int8_t(i >= T.n_orig[item] || j >= T.m_orig[item] ? pad_class : GTR_CLASS_NEGATIVE);
}

// one thread per pair: a plain store of the same value, so duplicates need no order; grid (ceil(kcap / 256), b)
__global__ __launch_bounds__(256) void gtr_target_pairs_kernel(const int32_t* __restrict__ pairs, int kcap, int8_t* __restrict__ cls, int n,
                                                               int m, TargetItems T) {
    const int item = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T.k[item]) return;
    const int i = pairs[(size_t(item) * 2 + 0) * kcap + t], j = pairs[(size_t(item) * 2 + 1) * kcap + t];
    if (i < 0 || j < 0 || i >= n || j >= m) return;                   // dropped (data_utils.py:216); negative: ignored
    if (i >= T.n_orig[item] || j >= T.m_orig[item]) return;           // the pad band overwrites it (:220-221)
    cls[(size_t(item) * n + i) * m + j] = GTR_CLASS_POSITIVE;
}

// one workgroup: how many pairs have a negative index
__global__ __launch_bounds__(256) void gtr_target_count_kernel(const int32_t* __restrict__ pairs, int b, int kcap, TargetItems T,
                                                               int32_t* __restrict__ negative_pairs) {
    __shared__ int wsum[4];
    int c = 0;
    for (int item = 0; item < b; ++item)
        for (int t = threadIdx.x; t < T.k[item]; t += 256)
            c += pairs[(size_t(item) * 2 + 0) * kcap + t] < 0 || pairs[(size_t(item) * 2 + 1) * kcap + t] < 0;
    c = wg::wave_sum(c);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) negative_pairs[0] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
int launch_status(const char* what) { return check_launch(-3, what, ": launch failed: "); }
bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int check_shape(int b, int n, int m) {
    if (b < 1 || b > GTR_MAX_BATCH) return fail(-1, "b must be in [1, %d] (got %d)", GTR_MAX_BATCH, b);
    if (n < 1 || m < 1) return fail(-1, "n, m must be >= 1 (got %d, %d)", n, m);
    if (n > GTR_MAX_POINTS || m > GTR_MAX_POINTS) return fail(-1, "at most %d points per side (got %d, %d)", GTR_MAX_POINTS, n, m);
    if (int64_t(n) * m > GTR_MAX_ELEMENTS) return fail(-1, "n * m must be <= %d (got %d x %d)", GTR_MAX_ELEMENTS, n, m);
    return 0;
}

int check_workspace(const Layout& L, const void* ws, size_t ws_bytes) {
    if (!ws) return fail(-1, "workspace is null");
    if (misaligned(ws, 256)) return fail(-1, "workspace must be 256-byte aligned");
    if (ws_bytes < L.total) return fail(-2, "workspace too small: %zu bytes, need %zu", ws_bytes, L.total);
    return 0;
}

int check_focal(double alpha, double gamma, double pos_w, double neg_w, Focal* f) {
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(-1, "alpha must be in [0, 1] (got %g)", alpha);
    if (!(gamma > 0.0) || std::isinf(gamma)) return fail(-1, "gamma must be finite and > 0 (got %g)", gamma);
    if (!(pos_w >= 0.0) || !(neg_w >= 0.0) || std::isinf(pos_w) || std::isinf(neg_w))
        return fail(-1, "pos_w and neg_w must be finite and >= 0 (got %g, %g)", pos_w, neg_w);
    *f = Focal{float(alpha), float(gamma), gamma == 2.0};
    return 0;
}

int check_scale(double scale) {
    if (!(scale >= 1.0 / 80.0) || std::isinf(scale)) return fail(-1, "scale must be finite and >= 1/80: exp(1 / scale) must not overflow (got %g)", scale);
    return 0;
}

template <class T>
T* at(char* ws, size_t off) { return reinterpret_cast<T*>(ws + off); }

int run_scores(const Layout& L, char* ws, const float* x, const float* y, double scale, float* r, int ldr, float* c, int ldc, bool with_yt,
               hipStream_t st) {
    hipLaunchKernelGGL(gtr_pack_kernel, dim3((std::max(L.ldn, L.ldm) / 4 + 255) / 256, D, 2 * L.b), dim3(256), 0, st, x, y,
                       at<float>(ws, L.px), at<float>(ws, L.py), L.b, L.n, L.m, L.ldn, L.ldm);
    if (with_yt) hipLaunchKernelGGL(gtr_pack_t_kernel, dim3(L.nct, D / 64, L.b), dim3(256), 0, st, y, at<float>(ws, L.pyt), L.m, L.ldm);
    if (int rc = launch_status("gtr pack")) return rc;
    ScoreArgs a{at<float>(ws, L.px), at<float>(ws, L.py), at<float>(ws, L.e), at<float>(ws, L.rowpart), at<float>(ws, L.colpart),
                L.n, L.m, L.ldn, L.ldm, L.nrt, L.nct, float(scale)};
    hipLaunchKernelGGL(gtr_score_exp_kernel, dim3(gatsspg::xcd_grid(L.nrt, L.nct), L.b), dim3(STile::THREADS),
                       sizeof(float) * STile::SMEM_FLOATS, st, a);
    hipLaunchKernelGGL(gtr_rc_kernel, dim3((L.n + L.m + 255) / 256, L.b), dim3(256), 0, st, a.rowpart, a.colpart, L.n, L.m, L.ldn, L.ldm,
                       L.nrt, L.nct, r, ldr, c, ldc);
    return launch_status("gtr score + exp");
}

PassArgs pass_args(const Layout& L, char* ws, const float* r, const float* c, int ldr, int ldc, const int8_t* cls, const Focal& f,
                   double pos_w, double neg_w) {
    PassArgs p{};
    p.E = at<float>(ws, L.e);
    p.r = r; p.c = c; p.ldr = ldr; p.ldc = ldc;
    p.cls = cls;
    p.n = L.n; p.m = L.m; p.ldn = L.ldn; p.ldm = L.ldm; p.nrt = L.nrt; p.nct = L.nct;
    p.cls4 = L.m % 4 == 0 && !misaligned(cls, 4);
    p.f = f; p.pos_w = float(pos_w); p.neg_w = float(neg_w);
    return p;
}

dim3 tile_grid(const Layout& L) { return dim3(unsigned(L.tiles), L.b); }

// terms + loss; with rowh / colh also the H sums
int run_terms(const Layout& L, char* ws, PassArgs p, double pos_w, double neg_w, double* loss_sums, int64_t* counts, float* loss, float* rowh,
              float* colh, hipStream_t st) {
    hipLaunchKernelGGL(gtr_terms_kernel, tile_grid(L), dim3(PT), 0, st, p, at<float2>(ws, L.hrow), at<float2>(ws, L.hcol),
                       at<float2>(ws, L.lsum), at<int4>(ws, L.lcnt));
    hipLaunchKernelGGL(gtr_loss_final_kernel, dim3(1), dim3(256), 0, st, at<float2>(ws, L.lsum), at<int4>(ws, L.lcnt), size_t(L.b) * L.tiles,
                       pos_w, neg_w, loss_sums, counts, loss);
    if (rowh) {
        p.counts = counts;
        hipLaunchKernelGGL(gtr_hsum_kernel, dim3((L.n + L.m + 255) / 256, L.b), dim3(256), 0, st, p, at<float2>(ws, L.hrow),
                           at<float2>(ws, L.hcol), rowh, colh);
    }
    return launch_status("gtr loss terms");
}

int run_copy(const float* src, size_t s_item, int s_ld, float* dst, size_t d_item, int d_ld, int b, int rows, int cols, hipStream_t st) {
    hipLaunchKernelGGL(gtr_copy_kernel, dim3(unsigned((size_t(rows) * cols + 255) / 256), b), dim3(256), 0, st, src, s_item, s_ld, dst, d_item,
                       d_ld, rows, cols);
    return launch_status("gtr copy");
}

}  // namespace

extern "C" {

int gtr_version(void) { return 1; }
const char* gtr_last_error(void) { return g_err; }

size_t gtr_workspace_bytes(int b, int n, int m) {
    if (check_shape(b, n, m)) return 0;
    return make_layout(b, n, m).total;
}

int gtr_build_target(const int32_t* pairs, const int32_t* k, const int32_t* n_orig, const int32_t* m_orig, int b, int kcap, int n, int m,
                     int pad_is_negative, int8_t* cls, int32_t* negative_pairs, void* stream) {
    if (int rc = check_shape(b, n, m)) return rc;
    if (kcap < 0) return fail(-1, "kcap must be >= 0 (got %d)", kcap);
    if (!k || !n_orig || !m_orig) return fail(-1, "k / n_orig / m_orig (host arrays) are null");
    if (!cls || (kcap > 0 && !pairs)) return fail(-1, "null argument");
    if (misaligned(pairs, 4) || misaligned(negative_pairs, 4)) return fail(-1, "misaligned argument");
    TargetItems T{};
    int kmax = 0;
    for (int i = 0; i < b; ++i) {
        if (k[i] < 0 || k[i] > kcap) return fail(-1, "item %d: k = %d is outside [0, kcap = %d]", i, k[i], kcap);
        if (n_orig[i] < 0 || m_orig[i] < 0) return fail(-1, "item %d: n_orig = %d, m_orig = %d must be >= 0", i, n_orig[i], m_orig[i]);
        T.k[i] = k[i]; T.n_orig[i] = n_orig[i]; T.m_orig[i] = m_orig[i];
        kmax = std::max(kmax, k[i]);
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(gtr_target_fill_kernel, dim3(unsigned((size_t(n) * m + 255) / 256), b), dim3(256), 0, st, cls, n, m,
                       pad_is_negative ? GTR_CLASS_NEGATIVE : GTR_CLASS_IGNORED, T);
    if (kmax > 0) hipLaunchKernelGGL(gtr_target_pairs_kernel, dim3((kmax + 255) / 256, b), dim3(256), 0, st, pairs, kcap, cls, n, m, T);
    if (negative_pairs) hipLaunchKernelGGL(gtr_target_count_kernel, dim3(1), dim3(256), 0, st, pairs, b, kcap, T, negative_pairs);
    return launch_status("gtr build target");
}

int gtr_loss_head(const float* x, const float* y, const int8_t* cls, int b, int n, int m, double alpha, double gamma, double pos_w,
                  double neg_w, double scale, float* loss, int64_t* counts, float* dx, float* dy, void* workspace, size_t workspace_bytes,
                  void* stream) {
    if (int rc = check_shape(b, n, m)) return rc;
    Focal f;
    if (int rc = check_focal(alpha, gamma, pos_w, neg_w, &f)) return rc;
    if (int rc = check_scale(scale)) return rc;
    const Layout L = make_layout(b, n, m);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    if (!x || !y || !cls || !loss || !counts) return fail(-1, "null argument");
    if ((dx == nullptr) != (dy == nullptr)) return fail(-1, "dx and dy must both be given or both be null");
    if (misaligned(x, 4) || misaligned(y, 4) || misaligned(loss, 4) || misaligned(counts, 8) || misaligned(dx, 4) || misaligned(dy, 4))
        return fail(-1, "misaligned argument");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *r = at<float>(ws, L.r), *c = at<float>(ws, L.c), *rowh = at<float>(ws, L.rowh), *colh = at<float>(ws, L.colh);
    if (int rc = run_scores(L, ws, x, y, scale, r, L.ldn, c, L.ldm, dx != nullptr, st)) return rc;
    PassArgs p = pass_args(L, ws, r, c, L.ldn, L.ldm, cls, f, pos_w, neg_w);
    if (int rc = run_terms(L, ws, p, pos_w, neg_w, nullptr, counts, loss, dx ? rowh : nullptr, colh, st)) return rc;
    if (!dx) return 0;
    p.counts = counts; p.rowh = rowh; p.colh = colh;
    hipLaunchKernelGGL(gtr_ds_kernel, tile_grid(L), dim3(PT), 0, st, p);
    const float inv_s = float(1.0 / scale);
    const size_t e_item = size_t(L.ldn) * L.ldm;
    // dx^T [n][256] = dS [n][ldm] y^T [ldm][256]
    GradArgs gx{p.E, at<float>(ws, L.pyt), e_item, size_t(L.ldm) * D, L.ldm, D, L.ldm / gatsspg::BK, L.nrt, D / BN, dx, n, inv_s};
    hipLaunchKernelGGL(gtr_grad_gemm_kernel<true>, dim3(gatsspg::xcd_grid(gx.nrt, gx.nct), b), dim3(GTile::THREADS),
                       sizeof(float) * GTile::SMEM_FLOATS, st, gx);
    // dy [256][m] = x [256][ldn] dS [ldn][ldm]
    GradArgs gy{at<float>(ws, L.px), p.E, size_t(D) * L.ldn, e_item, L.ldn, L.ldm, L.ldn / gatsspg::BK, D / BM, L.nct, dy, m, inv_s};
    hipLaunchKernelGGL(gtr_grad_gemm_kernel<false>, dim3(gatsspg::xcd_grid(gy.nrt, gy.nct), b), dim3(GTile::THREADS),
                       sizeof(float) * GTile::SMEM_FLOATS, st, gy);
    return launch_status("gtr score gradient");
}

int gtr_scores_exp(const float* x, const float* y, int b, int n, int m, double scale, float* E, float* r, float* c, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(b, n, m)) return rc;
    if (int rc = check_scale(scale)) return rc;
    const Layout L = make_layout(b, n, m);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    if (!x || !y || !E || !r || !c) return fail(-1, "null argument");
    if (misaligned(x, 4) || misaligned(y, 4) || misaligned(E, 4) || misaligned(r, 4) || misaligned(c, 4)) return fail(-1, "misaligned argument");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = run_scores(L, ws, x, y, scale, r, n, c, m, false, st)) return rc;
    return run_copy(at<float>(ws, L.e), size_t(L.ldn) * L.ldm, L.ldm, E, size_t(n) * m, m, b, n, m, st);
}

int gtr_loss_terms(const float* E, const float* r, const float* c, const int8_t* cls, int b, int n, int m, double alpha, double gamma,
                   double pos_w, double neg_w, double* loss_sums, int64_t* counts, float* loss, float* rowsum_h, float* colsum_h,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(b, n, m)) return rc;
    Focal f;
    if (int rc = check_focal(alpha, gamma, pos_w, neg_w, &f)) return rc;
    const Layout L = make_layout(b, n, m);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    if (!E || !r || !c || !cls || !loss_sums || !counts || !loss || !rowsum_h || !colsum_h) return fail(-1, "null argument");
    if (misaligned(E, 4) || misaligned(r, 4) || misaligned(c, 4) || misaligned(loss_sums, 8) || misaligned(counts, 8) || misaligned(loss, 4) ||
        misaligned(rowsum_h, 4) || misaligned(colsum_h, 4))
        return fail(-1, "misaligned argument");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = run_copy(E, size_t(n) * m, m, at<float>(ws, L.e), size_t(L.ldn) * L.ldm, L.ldm, b, n, m, st)) return rc;
    const PassArgs p = pass_args(L, ws, r, c, n, m, cls, f, pos_w, neg_w);
    return run_terms(L, ws, p, pos_w, neg_w, loss_sums, counts, loss, rowsum_h, colsum_h, st);
}

int gtr_score_grad(const float* E, const float* r, const float* c, const int8_t* cls, const int64_t* counts, const float* rowsum_h,
                   const float* colsum_h, int b, int n, int m, double alpha, double gamma, double pos_w, double neg_w, float* dS,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_shape(b, n, m)) return rc;
    Focal f;
    if (int rc = check_focal(alpha, gamma, pos_w, neg_w, &f)) return rc;
    const Layout L = make_layout(b, n, m);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    if (!E || !r || !c || !cls || !counts || !rowsum_h || !colsum_h || !dS) return fail(-1, "null argument");
    if (misaligned(E, 4) || misaligned(r, 4) || misaligned(c, 4) || misaligned(counts, 8) || misaligned(rowsum_h, 4) || misaligned(colsum_h, 4) ||
        misaligned(dS, 4))
        return fail(-1, "misaligned argument");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = run_copy(E, size_t(n) * m, m, at<float>(ws, L.e), size_t(L.ldn) * L.ldm, L.ldm, b, n, m, st)) return rc;
    PassArgs p = pass_args(L, ws, r, c, n, m, cls, f, pos_w, neg_w);
    p.counts = counts; p.rowh = rowsum_h; p.colh = colsum_h;
    hipLaunchKernelGGL(gtr_ds_kernel, tile_grid(L), dim3(PT), 0, st, p);
    if (int rc = launch_status("gtr score gradient")) return rc;
    return run_copy(at<float>(ws, L.e), size_t(L.ldn) * L.ldm, L.ldm, dS, size_t(n) * m, m, b, n, m, st);
}

}  // extern "C"
