// Nearest-neighbour matcher on gfx950 (include/superglue/nn_matcher.h): descriptor similarity fused with the top-2
// selection of both directions, then ratio / distance tests and the mutual check.  fp32 throughout: the contraction
// runs on v_mfma_f32_32x32x2_f32 through the main loop of gemm_f32_mfma.h, everything else on fp32 VALU.
//
// Three launches per call, whatever the batch:
//   nnm_pack_kernel      descriptors [256][n] -> planes [256][ld], ld padded to the tile and zero-filled, so that the
//                        main loop loads whole slabs;
//   nnm_sim_top2_kernel  one workgroup per (row tile, column tile, item): 128 x 64 tile of desc0^T desc1, reduced in the
//                        epilogue to {best, second, index of the best} per row and per column of the tile;
//   nnm_finalize_kernel  merges the partials in ascending tile order and applies the reference's tests.
// Every reduction runs in a fixed order that depends on the item's own counts alone (no atomics): two calls on the same
// inputs are bitwise identical, and an item of a ragged batch is bitwise the item alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../../include/superglue/nn_matcher.h"
#include "../capi_common.h"
#include "../gemm_f32_mfma.h"

namespace {

using namespace capi;
using gatsspg::f32x16;
using gatsspg::vf4;

constexpr int D = NNM_DESC_DIM;
// 128 x 64 on 8 waves (4 x 2 of 32 x 32), A operand K-major: the tile shape of the GATsSPG score contraction
using Tile = gatsspg::GemmTile<NNM_TILE_ROWS, NNM_TILE_COLS, 4, 2, true>;
constexpr int BM = Tile::BM, BN = Tile::BN;
constexpr int TS = BN + 1;                              // row stride of the staged tile: conflict-free column walks
constexpr int COLPART_OFF = BM * TS;                    // [3][THREADS / BN][BN] column part results behind the staged tile
static_assert(COLPART_OFF + 3 * Tile::THREADS <= Tile::SMEM_FLOATS, "the staged tile and the column parts must fit the operand buffers");
static_assert(D % (2 * gatsspg::BK) == 0, "the main loop takes an even number of slabs");

// ---- per-item counts (as superglue.hip's): by value in the kernel arguments, a uniform batch is entry 0 ----
struct Items {
    int n[2][NNM_MAX_ITEMS];
    int uniform;
    __host__ __device__ int count(int s, int bi) const { return n[s][uniform ? 0 : bi]; }
};

// Where everything lives: the planes and the partials are laid out by the capacities, addressed by (item, point, tile)
struct Layout {
    int b, cap0, cap1, ld0, ld1, nrt, nct;             // ld: padded leading dimensions; nrt / nct: tiles of the capacities
    size_t p0, p1, rowpart, colpart, total;            // byte offsets into the workspace
};

Layout make_layout(int b, int cap0, int cap1) {
    Layout L{};
    L.b = b; L.cap0 = cap0; L.cap1 = cap1;
    L.ld0 = round_up(cap0, BM); L.ld1 = round_up(cap1, BN);
    L.nrt = L.ld0 / BM; L.nct = L.ld1 / BN;
    Bump a(nullptr);
    L.p0 = a.reserve(sizeof(float) * size_t(b) * D * L.ld0);
    L.p1 = a.reserve(sizeof(float) * size_t(b) * D * L.ld1);
    L.rowpart = a.reserve(sizeof(float4) * size_t(b) * cap0 * L.nct);     // [item][row][column tile]
    L.colpart = a.reserve(sizeof(float4) * size_t(b) * cap1 * L.nrt);     // [item][column][row tile]
    L.total = a.off;
    return L;
}

// ---- running top 2 of a multiset of (value, index): best, its index (the lowest among equal values), and the second value of
// the multiset (== best when the maximum occurs twice).  Empty: (-inf, -inf, INT_MAX). ----
struct Top2 {
    float best, second;
    int idx;
};
__device__ __forceinline__ Top2 top2_empty() { return Top2{-INFINITY, -INFINITY, 0x7fffffff}; }
__device__ __forceinline__ void top2_push(Top2& t, float v, int j) {
    if (v > t.best || (v == t.best && j < t.idx)) { t.second = t.best; t.best = v; t.idx = j; }
    else if (v > t.second) t.second = v;
}
// merged in ascending index order this is "a later part wins with a strict > only"; the index comparison makes the order free
__device__ __forceinline__ void top2_merge(Top2& a, const Top2& b) {
    if (b.best > a.best || (b.best == a.best && b.idx < a.idx)) { a.second = fmaxf(a.best, b.second); a.best = b.best; a.idx = b.idx; }
    else a.second = fmaxf(a.second, b.best);
}
__device__ __forceinline__ float4 top2_pack(const Top2& t) { return make_float4(t.best, t.second, __int_as_float(t.idx), 0.f); }
__device__ __forceinline__ Top2 top2_unpack(const float4& v) { return Top2{v.x, v.y, __float_as_int(v.z)}; }

// ---- pack: plane z < b is side 0 of item z, plane b + i side 1 of item i (one plane, b, with shared1).  A thread moves four
// columns of one channel; columns past the plane's count are written as zeros up to ld. ----
__global__ __launch_bounds__(256) void nnm_pack_kernel(const float* __restrict__ d0, const float* __restrict__ d1, float* __restrict__ P0,
                                                       float* __restrict__ P1, int b, int cap0, int cap1, int ld0, int ld1, int n1_shared,
                                                       Items T) {
    const int z = blockIdx.z, k = blockIdx.y, side = z >= b, item = side ? z - b : z;
    const int cap = side ? cap1 : cap0, ld = side ? ld1 : ld0;
    const int n = side ? (n1_shared ? n1_shared : T.count(1, item)) : T.count(0, item);
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= ld) return;
    const float* src = (side ? d1 : d0) + (size_t(item) * D + k) * cap;
    vf4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c + j < n ? src[c + j] : 0.f;
    *reinterpret_cast<vf4*>((side ? P1 : P0) + (size_t(item) * D + k) * ld + c) = v;
}

// ---- similarity tile + top 2.  SIM: the tile is written to sim_out [n0][n1] instead of being reduced (nnm_similarity). ----
struct SimArgs {
    const float *P0, *P1;
    size_t s0, s1;                    // item strides of the planes in floats (s1 = 0: one shared plane)
    int cap0, cap1, ld0, ld1, nrt, nct;
    float4 *rowpart, *colpart;
    float* sim_out;
    Items items;
};

template <bool SIM>
__global__ __launch_bounds__(Tile::THREADS) void nnm_sim_top2_kernel(SimArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int rt, ct;
    if (!gatsspg::xcd_tile_map(p.nrt, p.nct, rt, ct)) return;
    const int item = blockIdx.y;
    const int n0 = p.items.count(0, item), n1 = p.items.count(1, item);
    if (rt * BM >= n0 || ct * BN >= n1) return;          // a tile past the item's own counts
    const int ld0 = p.ld0, ld1 = p.ld1;
    const float* Ap = p.P0 + item * p.s0 + rt * BM;      // K-major A: [256][ld0], the tile's 128 points contiguous
    const float* Bp = p.P1 + item * p.s1 + ct * BN;
    f32x16 acc[Tile::TM][Tile::TN];
    gatsspg::zero_acc(acc);
    gatsspg::gemm_mainloop<Tile>(
        acc, smem, D / gatsspg::BK, [&](int kt) { return Ap + size_t(kt) * gatsspg::BK * ld0; }, ld0,
        [&](int kt) { return Bp + size_t(kt) * gatsspg::BK * ld1; }, ld1);

    // the accumulators leave through LDS (free: the main loop ends on a barrier): staged tile [128][65]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / Tile::WN, wn = wave % Tile::WN, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) smem[(wm * 32 + gatsspg::mfma_row(r, half)) * TS + wn * 32 + l31] = acc[0][0][r];
    __syncthreads();
    const int rows = min(BM, n0 - rt * BM), cols = min(BN, n1 - ct * BN);   // the tile's valid extent: by index, never by value
    if constexpr (SIM) {
        for (int idx = tid; idx < BM * BN; idx += Tile::THREADS) {
            const int row = idx / BN, col = idx % BN;
            if (row < rows && col < cols) p.sim_out[size_t(rt * BM + row) * n1 + ct * BN + col] = smem[row * TS + col];
        }
        return;
    }
    // rows: four lanes per row, 16 consecutive columns each, merged in column order
    {
        constexpr int LPR = Tile::THREADS / BM, CPL = BN / LPR;
        const int row = tid / LPR, hp = tid % LPR;
        const float* tr = smem + row * TS + hp * CPL;
        Top2 t = top2_empty();
#pragma unroll
        for (int m = 0; m < CPL; ++m)
            if (hp * CPL + m < cols) top2_push(t, tr[m], ct * BN + hp * CPL + m);
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) {
            const Top2 u{__shfl_xor(t.best, o), __shfl_xor(t.second, o), __shfl_xor(t.idx, o)};
            top2_merge(t, u);
        }
        if (hp == 0 && row < rows) p.rowpart[(size_t(item) * p.cap0 + rt * BM + row) * p.nct + ct] = top2_pack(t);
    }
    // columns: eight groups of 16 rows, one thread per (group, column), then the groups in row order
    {
        constexpr int NQ = Tile::THREADS / BN, RPQ = BM / NQ;
        const int c = tid % BN, q = tid / BN;
        Top2 t = top2_empty();
#pragma unroll
        for (int m = 0; m < RPQ; ++m)
            if (q * RPQ + m < rows) top2_push(t, smem[(q * RPQ + m) * TS + c], rt * BM + q * RPQ + m);
        float* part = smem + COLPART_OFF;
        part[(0 * NQ + q) * BN + c] = t.best;
        part[(1 * NQ + q) * BN + c] = t.second;
        part[(2 * NQ + q) * BN + c] = __int_as_float(t.idx);
        __syncthreads();
        if (tid < cols) {
            Top2 a = top2_empty();
#pragma unroll
            for (int g = 0; g < NQ; ++g)
                top2_merge(a, Top2{part[(0 * NQ + g) * BN + tid], part[(1 * NQ + g) * BN + tid], __float_as_int(part[(2 * NQ + g) * BN + tid])});
            p.colpart[(size_t(item) * p.cap1 + ct * BN + tid) * p.nrt + rt] = top2_pack(a);
        }
    }
}

// ---- finalize: find_nn (reference :5-15) of a row or a column from its partials, then mutual_check (:18-23) ----
struct Tests {
    float ratio2, dist2;              // (float)(ratio^2), (float)(distance^2): the scalar the reference multiplies / compares in fp32
    int use_ratio, use_dist, mutual;
};
struct Found {
    int match;                        // -1 where a test fails
    float score;
};
// part: the element's partials [tiles of the capacity]; mine: tiles of the item's own count, merged in ascending order; n: points of the
// other side (a stray index -- NaN descriptors -- is brought into range)
__device__ __forceinline__ Found find_nn(const float4* __restrict__ part, int mine, int n, const Tests& ts) {
    Top2 t = top2_unpack(part[0]);
    for (int k = 1; k < mine; ++k) top2_merge(t, top2_unpack(part[k]));
    if (unsigned(t.idx) >= unsigned(n)) t.idx = 0;
    const float dist0 = 2.f * (1.f - t.best), dist1 = 2.f * (1.f - t.second);
    bool ok = true;
    if (ts.use_ratio) ok = ok && dist0 <= ts.ratio2 * dist1;
    if (ts.use_dist) ok = ok && dist0 <= ts.dist2;
    return Found{ok ? t.idx : -1, ok ? (t.best + 1.f) / 2.f : 0.f};
}

__global__ __launch_bounds__(256) void nnm_finalize_kernel(const float4* __restrict__ rowpart, const float4* __restrict__ colpart, int cap0,
                                                           int cap1, int nrt, int nct, Items T, Tests ts, int64_t* __restrict__ m0,
                                                           int64_t* __restrict__ m1, float* __restrict__ s0, float* __restrict__ s1) {
    const int item = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cap0 + cap1) return;
    const int n0 = T.count(0, item), n1 = T.count(1, item);
    const int my_nct = (n1 + BN - 1) / BN, my_nrt = (n0 + BM - 1) / BM;
    const float4* rp = rowpart + size_t(item) * cap0 * nct;
    const float4* cp = colpart + size_t(item) * cap1 * nrt;
    if (k < cap0) {
        Found f{-1, 0.f};
        if (k < n0) {
            f = find_nn(rp + size_t(k) * nct, my_nct, n1, ts);
            // the mutual check rewrites matches0 only: the score of a match it drops stays (the reference as written)
            if (ts.mutual && f.match >= 0 && find_nn(cp + size_t(f.match) * nrt, my_nrt, n0, ts).match != k) f.match = -1;
        }
        m0[size_t(item) * cap0 + k] = f.match;
        s0[size_t(item) * cap0 + k] = f.score;
    } else {
        const int j = k - cap0;
        Found f{-1, 0.f};
        if (j < n1) f = find_nn(cp + size_t(j) * nrt, my_nrt, n0, ts);
        m1[size_t(item) * cap1 + j] = f.match;
        s1[size_t(item) * cap1 + j] = f.score;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
int launch_status(const char* what) { return check_launch(-3, what, ": launch failed: "); }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}
bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int check_shape(int b, int cap0, int cap1) {
    if (b < 1 || b > NNM_MAX_ITEMS) return fail(-1, "b must be in [1, %d] (got %d)", NNM_MAX_ITEMS, b);
    if (cap0 < 1 || cap1 < 1) return fail(-1, "n0, n1 must be >= 1 (got %d, %d): an empty side has no nearest neighbour", cap0, cap1);
    if (cap0 > NNM_MAX_POINTS || cap1 > NNM_MAX_POINTS) return fail(-1, "at most %d points per side (got %d, %d)", NNM_MAX_POINTS, cap0, cap1);
    return 0;
}

int check_tests(double ratio, double distance, int mutual, const Items& items, int b, Tests* ts) {
    if (!(ratio >= 0.0) || !(distance >= 0.0) || std::isinf(ratio) || std::isinf(distance))
        return fail(-1, "ratio and distance thresholds must be finite and >= 0 (0 = no test; got %g, %g)", ratio, distance);
    if (ratio > 0.0)
        for (int i = 0; i < (items.uniform ? 1 : b); ++i)
            if (items.n[0][i] < 2 || items.n[1][i] < 2)
                return fail(-1, "item %d: the ratio test needs a second neighbour, n0 = %d and n1 = %d must be >= 2", i, items.n[0][i],
                            items.n[1][i]);
    *ts = Tests{float(ratio * ratio), float(distance * distance), ratio > 0.0, distance > 0.0, mutual != 0};
    return 0;
}

int check_workspace(const Layout& L, const void* ws, size_t ws_bytes) {
    if (!ws) return fail(-1, "workspace is null");
    if (misaligned(ws, 16)) return fail(-1, "workspace must be 16-byte aligned");
    if (ws_bytes < L.total) return fail(-2, "workspace too small: %zu bytes, need %zu", ws_bytes, L.total);
    return 0;
}

struct Outputs {
    int64_t *m0, *m1;
    float *s0, *s1;
};

// the inputs, the outputs and the workspace against each other
int check_buffers(const Layout& L, const float* desc0, const float* desc1, int planes1, const Outputs& o, const void* ws) {
    if (!desc0 || !desc1 || !o.m0 || !o.m1 || !o.s0 || !o.s1) return fail(-1, "null argument");
    const void* ptr[7] = {o.m0, o.m1, o.s0, o.s1, desc0, desc1, ws};
    const size_t size[7] = {sizeof(int64_t) * L.b * L.cap0, sizeof(int64_t) * L.b * L.cap1, sizeof(float) * L.b * L.cap0,
                            sizeof(float) * L.b * L.cap1, sizeof(float) * size_t(L.b) * D * L.cap0, sizeof(float) * size_t(planes1) * D * L.cap1,
                            L.total};
    const size_t align[7] = {8, 8, 4, 4, 4, 4, 16};
    static const char* const name[7] = {"matches0", "matches1", "matching_scores0", "matching_scores1", "desc0", "desc1", "workspace"};
    for (int i = 0; i < 7; ++i)
        if (misaligned(ptr[i], align[i])) return fail(-1, "%s is misaligned", name[i]);
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlap(ptr[i], size[i], ptr[j], size[j])) return fail(-1, "%s must not alias %s", name[i], name[j]);
    return 0;
}

SimArgs sim_args(const Layout& L, char* ws, const Items& items, int shared1) {
    SimArgs a{};
    a.P0 = reinterpret_cast<const float*>(ws + L.p0); a.P1 = reinterpret_cast<const float*>(ws + L.p1);
    a.s0 = size_t(D) * L.ld0; a.s1 = shared1 ? 0 : size_t(D) * L.ld1;
    a.cap0 = L.cap0; a.cap1 = L.cap1; a.ld0 = L.ld0; a.ld1 = L.ld1; a.nrt = L.nrt; a.nct = L.nct;
    a.rowpart = reinterpret_cast<float4*>(ws + L.rowpart); a.colpart = reinterpret_cast<float4*>(ws + L.colpart);
    a.items = items;
    return a;
}

int run_pack(const Layout& L, char* ws, const float* desc0, const float* desc1, const Items& items, int shared1, hipStream_t st) {
    int n1_shared = 0;                // the shared plane holds the columns some item reads
    if (shared1)
        for (int i = 0; i < L.b; ++i) n1_shared = std::max(n1_shared, items.count(1, i));
    const dim3 grid((std::max(L.ld0, L.ld1) / 4 + 255) / 256, D, L.b + (shared1 ? 1 : L.b));
    hipLaunchKernelGGL(nnm_pack_kernel, grid, dim3(256), 0, st, desc0, desc1, reinterpret_cast<float*>(ws + L.p0),
                       reinterpret_cast<float*>(ws + L.p1), L.b, L.cap0, L.cap1, L.ld0, L.ld1, n1_shared, items);
    return launch_status("nnm pack");
}

template <bool SIM>
int run_sim(const Layout& L, const SimArgs& a, hipStream_t st) {
    const dim3 grid(gatsspg::xcd_grid(L.nrt, L.nct), L.b);
    hipLaunchKernelGGL(nnm_sim_top2_kernel<SIM>, grid, dim3(Tile::THREADS), sizeof(float) * Tile::SMEM_FLOATS, st, a);
    return launch_status(SIM ? "nnm similarity" : "nnm similarity + top 2");
}

// nnm_match and nnm_match_ragged on checked arguments: they differ in the table alone
int run_match(const Layout& L, const float* desc0, const float* desc1, const Items& items, int shared1, const Tests& ts, const Outputs& o,
              void* workspace, sg_stream_t stream) {
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = run_pack(L, ws, desc0, desc1, items, shared1, st)) return rc;
    const SimArgs a = sim_args(L, ws, items, shared1);
    if (int rc = run_sim<false>(L, a, st)) return rc;
    hipLaunchKernelGGL(nnm_finalize_kernel, dim3((L.cap0 + L.cap1 + 255) / 256, L.b), dim3(256), 0, st, a.rowpart, a.colpart, L.cap0, L.cap1,
                       L.nrt, L.nct, items, ts, o.m0, o.m1, o.s0, o.s1);
    return launch_status("nnm finalize");
}

}  // namespace

extern "C" {

size_t nnm_workspace_bytes(int b, int cap0, int cap1) {
    if (check_shape(b, cap0, cap1)) return 0;
    return make_layout(b, cap0, cap1).total;
}

int nnm_match(const float* desc0, const float* desc1, int b, int n0, int n1, double ratio, double distance, int mutual, int64_t* matches0,
              int64_t* matches1, float* mscores0, float* mscores1, void* workspace, size_t workspace_bytes, sg_stream_t stream, int flags) {
    if (flags) return fail(-1, "flags must be 0 (got %#x): this matcher has one arithmetic, fp32", unsigned(flags));
    if (int rc = check_shape(b, n0, n1)) return rc;
    Items items{};
    items.uniform = 1; items.n[0][0] = n0; items.n[1][0] = n1;
    Tests ts;
    if (int rc = check_tests(ratio, distance, mutual, items, b, &ts)) return rc;
    const Layout L = make_layout(b, n0, n1);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    const Outputs o{matches0, matches1, mscores0, mscores1};
    if (int rc = check_buffers(L, desc0, desc1, b, o, workspace)) return rc;
    return run_match(L, desc0, desc1, items, 0, ts, o, workspace, stream);
}

int nnm_match_ragged(const float* desc0, const float* desc1, const int32_t* n0, const int32_t* n1, int b, int cap0, int cap1, int shared1,
                     double ratio, double distance, int mutual, int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                     void* workspace, size_t workspace_bytes, sg_stream_t stream, int flags) {
    if (flags) return fail(-1, "flags must be 0 (got %#x): this matcher has one arithmetic, fp32", unsigned(flags));
    if (int rc = check_shape(b, cap0, cap1)) return rc;
    if (!n0 || !n1) return fail(-1, "n0 / n1 (host arrays) are null");
    Items items{};
    for (int i = 0; i < b; ++i) {
        if (n0[i] < 1 || n0[i] > cap0) return fail(-1, "item %d: n0 = %d is outside [1, cap0 = %d]", i, n0[i], cap0);
        if (n1[i] < 1 || n1[i] > cap1) return fail(-1, "item %d: n1 = %d is outside [1, cap1 = %d]", i, n1[i], cap1);
        items.n[0][i] = n0[i]; items.n[1][i] = n1[i];
    }
    Tests ts;
    if (int rc = check_tests(ratio, distance, mutual, items, b, &ts)) return rc;
    const Layout L = make_layout(b, cap0, cap1);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    const Outputs o{matches0, matches1, mscores0, mscores1};
    if (int rc = check_buffers(L, desc0, desc1, shared1 ? 1 : b, o, workspace)) return rc;
    return run_match(L, desc0, desc1, items, shared1 != 0, ts, o, workspace, stream);
}

int nnm_similarity(const float* desc0, const float* desc1, int n0, int n1, float* sim_out, void* workspace, size_t workspace_bytes,
                   sg_stream_t stream, int flags) {
    if (flags) return fail(-1, "flags must be 0 (got %#x): this matcher has one arithmetic, fp32", unsigned(flags));
    if (int rc = check_shape(1, n0, n1)) return rc;
    const Layout L = make_layout(1, n0, n1);
    if (int rc = check_workspace(L, workspace, workspace_bytes)) return rc;
    if (!desc0 || !desc1 || !sim_out) return fail(-1, "null argument");
    if (misaligned(desc0, 4) || misaligned(desc1, 4) || misaligned(sim_out, 4)) return fail(-1, "misaligned argument");
    const size_t out_bytes = sizeof(float) * size_t(n0) * n1;
    if (overlap(sim_out, out_bytes, desc0, sizeof(float) * size_t(D) * n0) || overlap(sim_out, out_bytes, desc1, sizeof(float) * size_t(D) * n1) ||
        overlap(sim_out, out_bytes, workspace, L.total))
        return fail(-1, "sim_out must not alias the inputs or the workspace");
    Items items{};
    items.uniform = 1; items.n[0][0] = n0; items.n[1][0] = n1;
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = run_pack(L, ws, desc0, desc1, items, 0, st)) return rc;
    SimArgs a = sim_args(L, ws, items, 0);
    a.sim_out = sim_out;
    return run_sim<true>(L, a, st);
}

}  // extern "C"
