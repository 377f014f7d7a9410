// Training-set builder of the GATsSPG matcher on gfx950 (include/gatsspg_trainset.h): ground-truth pairs per image, leaf
// selection and gather, query and database padding.  Integer arithmetic and copies only: no value is computed in floating point
// but the pads, which are exact.
//
// Launches of gts_build_batch (the header states the rules):
//   gts_select_kernel        one thread per (sample, 3D point): the point's num_leaf slots into leaf_src (workspace);
//   gts_gather_kernel        one workgroup per 64 leaves x 64 channels of one sample: rows of collect -> LDS -> columns of the
//                            batch.  Both global sides move 16 bytes per lane in 256-byte runs; the tile is stored with its
//                            column quads XOR-swizzled by the channel quad, so that the 4-byte LDS stores are 2-way (free on a
//                            ds_write_b32) and the 16-byte LDS reads conflict-free;
//   gts_pad_query_kernel     descriptor, score and keypoint copies of the query side, ones / zeros behind them;
//   gts_pad_kpts_kernel      the random keypoints behind the image's own, compared with those through LDS;
//   gts_pad_points_kernel    the 3D side: mean descriptors, points, pads.
// gts_assign_pairs: init | claim (a minimum per keypoint) | one-workgroup scan over the keypoints | emit.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/gatsspg_trainset.h"
#include "capi_common.h"
#include "ransac_sample.h"
#include "wg_primitives.h"

namespace {

using namespace capi;
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int D = GTS_DESC_DIM;
constexpr int NT = 256;          // threads of every kernel here but the scan
constexpr int TILE = 64;         // leaves and channels of a gather tile
constexpr int SCAN_NT = 1024;
static_assert(D % TILE == 0, "whole channel tiles");

__device__ __forceinline__ u64 stream_key(u64 seed, u64 tag, int epoch, int image, int item) {
    u64 h = sampling::splitmix64(seed);
    h = sampling::splitmix64(h ^ tag);
    h = sampling::splitmix64(h ^ u64(uint32_t(epoch)));
    h = sampling::splitmix64(h ^ u64(uint32_t(image)));
    return sampling::splitmix64(h ^ u64(uint32_t(item)));
}
__device__ __forceinline__ u64 draw64(u64 key, u64 ctr) { return sampling::splitmix64(key + ctr); }
__device__ __forceinline__ int draw_index(u64 key, u64 ctr, int n) { return int((draw64(key, ctr) >> 11) % u64(n)); }

// ---- ground-truth pairs ----
__global__ __launch_bounds__(NT) void gts_assign_init_kernel(int32_t* owner, int G, int32_t* ignored) {
    const int g = blockIdx.x * NT + threadIdx.x;
    if (g < G) owner[g] = INT_MAX;
    if (g == 0) *ignored = 0;
}

// one thread per point: each of its observations that is the lowest keypoint of the point in its image claims that keypoint
__global__ __launch_bounds__(NT) void gts_assign_claim_kernel(const int32_t* __restrict__ point_offsets, const int32_t* __restrict__ obs_image,
                                                              const int32_t* __restrict__ obs_kpt, int N, int K,
                                                              const int32_t* __restrict__ kpt_offsets, int V, int G, int32_t* owner,
                                                              int32_t* ignored) {
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= N) return;
    const int s = max(point_offsets[p], 0), e = min(point_offsets[p + 1], K);
    for (int j = s; j < e; ++j) {
        const int v = obs_image[j], q = obs_kpt[j];
        int off = 0, nv = 0;
        if (v >= 0 && v < V) {
            off = kpt_offsets[v];
            nv = kpt_offsets[v + 1] - off;
        }
        if (q < 0 || q >= nv || off < 0 || off + q >= G) {
            atomicAdd(ignored, 1);
            continue;
        }
        bool winner = true;
        for (int j2 = s; j2 < e; ++j2) {
            const int q2 = obs_kpt[j2];
            if (j2 != j && obs_image[j2] == v && q2 >= 0 && q2 < nv && (q2 < q || (q2 == q && j2 < j))) winner = false;
        }
        if (winner) atomicMin(&owner[off + q], p);
    }
}

// scanv[g] = the claimed keypoints before g, scanv[G] = their number: one workgroup, chunk after chunk
__global__ __launch_bounds__(SCAN_NT) void gts_assign_scan_kernel(const int32_t* __restrict__ owner, int G, int32_t* __restrict__ scanv) {
    __shared__ int wsum[SCAN_NT / 64];
    int carry = 0;
    for (int base = 0; base < G; base += SCAN_NT) {
        const int g = base + threadIdx.x;
        const int f = g < G && owner[g] != INT_MAX;
        int total;
        const int before = wg::excl_scan<SCAN_NT>(f, wsum, total);
        if (g < G) scanv[g] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) scanv[G] = carry;
}

__global__ __launch_bounds__(NT) void gts_assign_emit_kernel(const int32_t* __restrict__ owner, const int32_t* __restrict__ scanv,
                                                             const int32_t* __restrict__ kpt_offsets, int V, int G, int K,
                                                             int32_t* __restrict__ pair_offsets, int32_t* __restrict__ pair_kpt,
                                                             int32_t* __restrict__ pair_point) {
    const int g = blockIdx.x * NT + threadIdx.x;
    if (g <= V) pair_offsets[g] = scanv[min(max(kpt_offsets[g], 0), G)];
    if (g >= G || owner[g] == INT_MAX) return;
    int lo = 0, hi = V;                      // the last image whose first keypoint is <= g (images without keypoints are passed over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kpt_offsets[mid] <= g) lo = mid; else hi = mid;
    }
    const int pos = scanv[g];
    if (pos < K) {
        pair_kpt[pos] = g - kpt_offsets[lo];
        pair_point[pos] = owner[g];
    }
}

// ---- leaves ----
// leaf_src is read back by the thread that wrote it (the distinctness test of the cnt >= L arm): not __restrict__
__global__ __launch_bounds__(NT) void gts_select_kernel(const int32_t* __restrict__ point_offsets, int N, const int32_t* __restrict__ sample_image,
                                                        const int32_t* __restrict__ sample_epoch, int shape3d, int L, u64 seed,
                                                        int32_t* leaf_src) {
    const int p = blockIdx.x * NT + threadIdx.x, s = blockIdx.y;
    if (p >= shape3d) return;
    int32_t* out = leaf_src + (size_t(s) * shape3d + p) * L;
    int start = 0, cnt = 0;
    if (p < N) {
        start = point_offsets[p];
        cnt = max(point_offsets[p + 1] - start, 0);
    }
    const u64 key = stream_key(seed, GTS_TAG_LEAVES, sample_epoch[s], sample_image[s], p);
    u64 ctr = 0;
    if (cnt < L) {
        for (int l = 0; l < L; ++l) out[l] = -1;
        u64 used = 0;
        for (int j = 0; j < cnt; ++j) {
            int slot;
            do slot = draw_index(key, ctr++, L); while ((used >> slot) & 1);
            used |= u64(1) << slot;
            out[slot] = start + j;
        }
    } else {
        for (int l = 0; l < L; ++l) {
            int v;
            bool dup;
            do {
                v = start + draw_index(key, ctr++, cnt);
                dup = false;
                for (int q = 0; q < l; ++q) dup |= out[q] == v;
            } while (dup);
            out[l] = v;
        }
    }
}

// grid (ceil(M / 64), 256 / 64, b).  Element (channel k, leaf c) of the tile lives at k * 64 + (c ^ ((k >> 2) << 2)).
template <bool VEC>
__global__ __launch_bounds__(NT) void gts_gather_kernel(const float* __restrict__ collect, int K, const int32_t* __restrict__ leaf_src, int M,
                                                        float* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float tile[TILE * TILE];
    const int t = threadIdx.x, c0 = blockIdx.x * TILE, kc = blockIdx.y * TILE, s = blockIdx.z;
    const int32_t* src = leaf_src + size_t(s) * M;
    {   // 16 lanes read the 256 bytes of one leaf's channel run: a wave takes four leaves an instruction
        const int kq = t & 15, cl = t >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 16 + cl, col = c0 + c;
            vf4 v = {1.f, 1.f, 1.f, 1.f};
            if (col < M) {
                const int r = src[col];
                if (r >= 0 && r < K) v = *reinterpret_cast<const vf4*>(collect + size_t(r) * D + kc + 4 * kq);
            }
            const int pc = c ^ (kq << 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(4 * kq + j) * TILE + pc] = v[j];
        }
    }
    __syncthreads();
    {   // 16 lanes write the 256 bytes of one channel's 64 leaves: a wave takes the four channels of one quad an instruction
        const int cq = t & 15, kr = t >> 4, col = c0 + 4 * cq;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = i * 16 + kr;
            const vf4 v = *reinterpret_cast<const vf4*>(&tile[k * TILE + 4 * (cq ^ (k >> 2))]);
            float* out = dst + (size_t(s) * D + kc + k) * M + col;
            if (VEC) {
                if (col < M) *reinterpret_cast<vf4*>(out) = v;      // M % 4 == 0: a quad is inside or outside as a whole
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (col + j < M) out[j] = v[j];
            }
        }
    }
}

// ---- padding ----
struct ImageInfo {
    int off, nv, h, w;
};
__device__ __forceinline__ ImageInfo image_info(const int32_t* kpt_offsets, const int32_t* image_hw, int V, int v) {
    ImageInfo I{0, 0, 1, 1};
    if (v >= 0 && v < V) {
        I.off = kpt_offsets[v];
        I.nv = max(kpt_offsets[v + 1] - I.off, 0);
        I.h = max(image_hw[2 * v], 1);
        I.w = max(image_hw[2 * v + 1], 1);
    }
    return I;
}

// grid (ceil(shape2d / 256), 257, b): y < 256 is a descriptor channel, y == 256 the scores and the image's own keypoints
__global__ __launch_bounds__(NT) void gts_pad_query_kernel(const float* __restrict__ desc2d, const float* __restrict__ kpts2d,
                                                           const float* __restrict__ scores2d, const int32_t* __restrict__ kpt_offsets,
                                                           const int32_t* __restrict__ image_hw, int V, const int32_t* __restrict__ sample_image,
                                                           int shape2d, float* __restrict__ dq, float* __restrict__ kq, float* __restrict__ sq) {
    const int j = blockIdx.x * NT + threadIdx.x, k = blockIdx.y, s = blockIdx.z;
    if (j >= shape2d) return;
    const ImageInfo I = image_info(kpt_offsets, image_hw, V, sample_image[s]);
    if (k < D) {
        dq[(size_t(s) * D + k) * shape2d + j] = j < I.nv ? desc2d[size_t(I.off) * D + size_t(k) * I.nv + j] : 1.f;
        return;
    }
    if (sq) sq[size_t(s) * shape2d + j] = j < I.nv ? scores2d[size_t(I.off) + j] : 0.f;
    if (j < I.nv) {
        float* o = kq + (size_t(s) * shape2d + j) * 2;
        o[0] = kpts2d[(size_t(I.off) + j) * 2];
        o[1] = kpts2d[(size_t(I.off) + j) * 2 + 1];
    }
}

// grid (ceil(shape2d / 256), b).  Every workgroup walks the image's keypoints through LDS, 256 at a time, once per attempt that
// one of its columns still needs.
__global__ __launch_bounds__(NT) void gts_pad_kpts_kernel(const float* __restrict__ kpts2d, const int32_t* __restrict__ kpt_offsets,
                                                          const int32_t* __restrict__ image_hw, int V, const int32_t* __restrict__ sample_image,
                                                          const int32_t* __restrict__ sample_epoch, int shape2d, u64 seed, float* __restrict__ kq) {
    __shared__ float2 kp[NT];
    const int t = threadIdx.x, j = blockIdx.x * NT + t, s = blockIdx.y;
    const int image = sample_image[s];
    const ImageInfo I = image_info(kpt_offsets, image_hw, V, image);
    if (blockIdx.x * NT + NT <= I.nv) return;                        // the whole workgroup is inside the copied part
    bool pending = j < shape2d && j >= I.nv;
    const u64 key = stream_key(seed, GTS_TAG_PAD2D, sample_epoch[s], image, j);
    for (int attempt = 0; attempt < GTS_MAX_REDRAWS; ++attempt) {
        float c0 = 0.f, c1 = 0.f;
        if (pending) {
            c0 = float(draw_index(key, 2 * u64(attempt), I.h));
            c1 = float(draw_index(key, 2 * u64(attempt) + 1, I.w));
        }
        bool hit = false;
        for (int base = 0; base < I.nv; base += NT) {
            __syncthreads();
            if (base + t < I.nv) kp[t] = reinterpret_cast<const float2*>(kpts2d)[size_t(I.off) + base + t];
            __syncthreads();
            if (pending) {
                const int m = min(NT, I.nv - base);
                for (int q = 0; q < m; ++q) hit |= kp[q].x == c0 && kp[q].y == c1;
            }
        }
        if (pending && (!hit || attempt == GTS_MAX_REDRAWS - 1)) {
            float* o = kq + (size_t(s) * shape2d + j) * 2;
            o[0] = c0;
            o[1] = c1;
            pending = false;
        }
        if (!__syncthreads_or(pending)) break;
    }
}

// grid (ceil(shape3d / 256), 257, b): y < 256 is a descriptor channel, y == 256 the points
__global__ __launch_bounds__(NT) void gts_pad_points_kernel(const float* __restrict__ points3d, const float* __restrict__ mean_desc, int N,
                                                            const int32_t* __restrict__ sample_image, const int32_t* __restrict__ sample_epoch,
                                                            int shape3d, u64 seed, float* __restrict__ k3, float* __restrict__ d3) {
    const int j = blockIdx.x * NT + threadIdx.x, k = blockIdx.y, s = blockIdx.z;
    if (j >= shape3d) return;
    if (k < D) {
        d3[(size_t(s) * D + k) * shape3d + j] = j < N ? mean_desc[size_t(k) * N + j] : 1.f;
        return;
    }
    float* o = k3 + (size_t(s) * shape3d + j) * 3;
    if (j < N) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = points3d[size_t(j) * 3 + c];
        return;
    }
    const u64 key = stream_key(seed, GTS_TAG_PAD3D, sample_epoch[s], sample_image[s], j);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = float(draw64(key, c) >> 40) * 0x1p-24f - 0.5f;      // a 24-bit integer: exact in fp32
}

// ---- host side ----
hipStream_t as_stream(gts_stream_t q) { return static_cast<hipStream_t>(q); }

bool misaligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int check_batch(const char* who, int b) {
    if (b < 1 || b > GTS_MAX_BATCH) return fail(-1, "%s: b must be in [1, %d] (got %d)", who, GTS_MAX_BATCH, b);
    return 0;
}

int check_side(const char* who, const char* what, int v) {
    if (v < 1 || v > GTS_MAX_POINTS) return fail(-1, "%s: %s must be in [1, %d] (got %d)", who, what, GTS_MAX_POINTS, v);
    return 0;
}

int check_leaves(const char* who, int shape3d, int num_leaf) {
    if (int rc = check_side(who, "shape3d", shape3d)) return rc;
    if (num_leaf < 1 || num_leaf > GTS_MAX_LEAF) return fail(-1, "%s: num_leaf must be in [1, %d] (got %d)", who, GTS_MAX_LEAF, num_leaf);
    if (size_t(shape3d) * num_leaf > GTS_MAX_COLUMNS)
        return fail(-1, "%s: shape3d * num_leaf must be <= %d (got %d * %d)", who, GTS_MAX_COLUMNS, shape3d, num_leaf);
    return 0;
}

int check_count(const char* who, const char* what, int v) {
    if (v < 1) return fail(-1, "%s: %s must be >= 1 (got %d)", who, what, v);
    return 0;
}

struct Layout {
    size_t owner, scanv, leaf_src, total;
};

Layout make_layout(int total_kpts, int b, int shape3d, int num_leaf) {
    Layout L{};
    Bump assign(nullptr), batch(nullptr);
    L.owner = assign.reserve(sizeof(int32_t) * size_t(total_kpts));
    L.scanv = assign.reserve(sizeof(int32_t) * (size_t(total_kpts) + 1));
    L.leaf_src = batch.reserve(sizeof(int32_t) * size_t(b) * shape3d * num_leaf);
    L.total = assign.off > batch.off ? assign.off : batch.off;      // the two calls do not overlap in time: one region
    return L;
}

int launch_select(const int32_t* point_offsets, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape3d, int num_leaf,
                  uint64_t seed, int32_t* leaf_src, hipStream_t st) {
    gts_select_kernel<<<dim3(ceil_div(shape3d, NT), b), NT, 0, st>>>(point_offsets, N, sample_image, sample_epoch, shape3d, num_leaf, seed, leaf_src);
    return check_launch(-3, "gts_select_kernel");
}

int launch_gather(const float* collect, int K, const int32_t* leaf_src, int b, int M, float* dst, hipStream_t st) {
    const dim3 grid(ceil_div(M, TILE), D / TILE, b);
    if (M % 4 == 0 && !misaligned(dst, 16))
        gts_gather_kernel<true><<<grid, NT, 0, st>>>(collect, K, leaf_src, M, dst);
    else
        gts_gather_kernel<false><<<grid, NT, 0, st>>>(collect, K, leaf_src, M, dst);
    return check_launch(-3, "gts_gather_kernel");
}

int launch_pad_query(const float* desc2d, const float* kpts2d, const float* scores2d, const int32_t* kpt_offsets, const int32_t* image_hw, int V,
                     const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape2d, uint64_t seed, float* dq, float* kq, float* sq,
                     hipStream_t st) {
    gts_pad_query_kernel<<<dim3(ceil_div(shape2d, NT), D + 1, b), NT, 0, st>>>(desc2d, kpts2d, scores2d, kpt_offsets, image_hw, V, sample_image,
                                                                               shape2d, dq, kq, sq);
    if (int rc = check_launch(-3, "gts_pad_query_kernel")) return rc;
    gts_pad_kpts_kernel<<<dim3(ceil_div(shape2d, NT), b), NT, 0, st>>>(kpts2d, kpt_offsets, image_hw, V, sample_image, sample_epoch, shape2d, seed,
                                                                       kq);
    return check_launch(-3, "gts_pad_kpts_kernel");
}

int launch_pad_points(const float* points3d, const float* mean_desc, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b,
                      int shape3d, uint64_t seed, float* k3, float* d3, hipStream_t st) {
    gts_pad_points_kernel<<<dim3(ceil_div(shape3d, NT), D + 1, b), NT, 0, st>>>(points3d, mean_desc, N, sample_image, sample_epoch, shape3d, seed,
                                                                                k3, d3);
    return check_launch(-3, "gts_pad_points_kernel");
}

#define GTS_NOT_NULL(who, ...)                                                          \
    do {                                                                                \
        const void* ptrs_[] = {__VA_ARGS__};                                            \
        for (const void* p_ : ptrs_) {                                                  \
            if (!p_) return fail(-1, "%s: a required pointer is null", who);            \
            if (misaligned(p_, 4)) return fail(-1, "%s: a pointer is misaligned", who); \
        }                                                                               \
    } while (0)

}  // namespace

extern "C" {

int gts_version(void) { return 1; }
const char* gts_last_error(void) { return g_err; }

size_t gts_workspace_bytes(int total_kpts, int b, int shape3d, int num_leaf) {
    const char* who = "gts_workspace_bytes";
    if (total_kpts < 0) return size_t(fail(0, "%s: total_kpts must be >= 0 (got %d)", who, total_kpts));
    if (b < 0 || b > GTS_MAX_BATCH) return size_t(fail(0, "%s: b must be in [0, %d] (got %d)", who, GTS_MAX_BATCH, b));
    if (b > 0 && check_leaves(who, shape3d, num_leaf)) return 0;
    if (b == 0 && total_kpts == 0) return size_t(fail(0, "%s: nothing to size: total_kpts and b are both 0", who));
    const Layout L = b > 0 ? make_layout(total_kpts, b, shape3d, num_leaf) : make_layout(total_kpts, 0, 0, 0);
    return L.total > 256 ? L.total : 256;
}

int gts_assign_pairs(const int32_t* point_offsets, const int32_t* obs_image, const int32_t* obs_kpt, int N, int K, const int32_t* kpt_offsets,
                     int V, int total_kpts, int32_t* pair_offsets, int32_t* pair_kpt, int32_t* pair_point, int32_t* ignored, void* workspace,
                     size_t workspace_bytes, gts_stream_t queue) {
    const char* who = "gts_assign_pairs";
    if (check_count(who, "N", N) || check_count(who, "K", K) || check_count(who, "V", V) || check_count(who, "total_kpts", total_kpts)) return -1;
    GTS_NOT_NULL(who, point_offsets, obs_image, obs_kpt, kpt_offsets, pair_offsets, pair_kpt, pair_point, ignored);
    const Layout L = make_layout(total_kpts, 0, 0, 0);
    if (int rc = check_workspace(who, workspace, workspace_bytes, L.total)) return rc;
    char* ws = static_cast<char*>(workspace);
    int32_t* owner = reinterpret_cast<int32_t*>(ws + L.owner);
    int32_t* scanv = reinterpret_cast<int32_t*>(ws + L.scanv);
    hipStream_t st = as_stream(queue);
    const int G = total_kpts;
    gts_assign_init_kernel<<<ceil_div(G, NT), NT, 0, st>>>(owner, G, ignored);
    gts_assign_claim_kernel<<<ceil_div(N, NT), NT, 0, st>>>(point_offsets, obs_image, obs_kpt, N, K, kpt_offsets, V, G, owner, ignored);
    gts_assign_scan_kernel<<<1, SCAN_NT, 0, st>>>(owner, G, scanv);
    gts_assign_emit_kernel<<<ceil_div(G > V + 1 ? G : V + 1, NT), NT, 0, st>>>(owner, scanv, kpt_offsets, V, G, K, pair_offsets, pair_kpt, pair_point);
    return check_launch(-3, "gts_assign_pairs");
}

int gts_select_leaves(const int32_t* point_offsets, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape3d,
                      int num_leaf, uint64_t seed, int32_t* leaf_src, gts_stream_t queue) {
    const char* who = "gts_select_leaves";
    if (check_batch(who, b) || check_leaves(who, shape3d, num_leaf) || check_count(who, "N", N)) return -1;
    GTS_NOT_NULL(who, point_offsets, sample_image, sample_epoch, leaf_src);
    return launch_select(point_offsets, N, sample_image, sample_epoch, b, shape3d, num_leaf, seed, leaf_src, as_stream(queue));
}

int gts_gather_leaves(const float* collect, int K, const int32_t* leaf_src, int b, int shape3d, int num_leaf, float* descriptors2d_db,
                      gts_stream_t queue) {
    const char* who = "gts_gather_leaves";
    if (check_batch(who, b) || check_leaves(who, shape3d, num_leaf) || check_count(who, "K", K)) return -1;
    GTS_NOT_NULL(who, collect, leaf_src, descriptors2d_db);
    if (misaligned(collect, 16)) return fail(-1, "%s: collect must be 16-byte aligned", who);
    return launch_gather(collect, K, leaf_src, b, shape3d * num_leaf, descriptors2d_db, as_stream(queue));
}

int gts_pad_query(const float* desc2d, const float* kpts2d, const float* scores2d, const int32_t* kpt_offsets, const int32_t* image_hw, int V,
                  const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape2d, uint64_t seed, float* descriptors2d_query,
                  float* keypoints2d, float* scores_query, gts_stream_t queue) {
    const char* who = "gts_pad_query";
    if (check_batch(who, b) || check_side(who, "shape2d", shape2d) || check_count(who, "V", V)) return -1;
    GTS_NOT_NULL(who, desc2d, kpts2d, scores2d, kpt_offsets, image_hw, sample_image, sample_epoch, descriptors2d_query, keypoints2d);
    if (misaligned(kpts2d, 8)) return fail(-1, "%s: kpts2d must be 8-byte aligned", who);
    if (misaligned(scores_query, 4)) return fail(-1, "%s: a pointer is misaligned", who);
    return launch_pad_query(desc2d, kpts2d, scores2d, kpt_offsets, image_hw, V, sample_image, sample_epoch, b, shape2d, seed, descriptors2d_query,
                            keypoints2d, scores_query, as_stream(queue));
}

int gts_pad_points(const float* points3d, const float* mean_desc, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b,
                   int shape3d, uint64_t seed, float* keypoints3d, float* descriptors3d_db, gts_stream_t queue) {
    const char* who = "gts_pad_points";
    if (check_batch(who, b) || check_side(who, "shape3d", shape3d) || check_count(who, "N", N)) return -1;
    GTS_NOT_NULL(who, points3d, mean_desc, sample_image, sample_epoch, keypoints3d, descriptors3d_db);
    return launch_pad_points(points3d, mean_desc, N, sample_image, sample_epoch, b, shape3d, seed, keypoints3d, descriptors3d_db, as_stream(queue));
}

int gts_build_batch(const int32_t* point_offsets, const float* collect, const float* points3d, const float* mean_desc, int N, int K,
                    const float* desc2d, const float* kpts2d, const float* scores2d, const int32_t* kpt_offsets, const int32_t* image_hw, int V,
                    const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape2d, int shape3d, int num_leaf, uint64_t seed,
                    float* descriptors2d_query, float* keypoints2d, float* scores_query, float* keypoints3d, float* descriptors3d_db,
                    float* descriptors2d_db, void* workspace, size_t workspace_bytes, gts_stream_t queue) {
    const char* who = "gts_build_batch";
    if (check_batch(who, b) || check_side(who, "shape2d", shape2d) || check_leaves(who, shape3d, num_leaf) || check_count(who, "N", N) ||
        check_count(who, "K", K) || check_count(who, "V", V))
        return -1;
    GTS_NOT_NULL(who, point_offsets, collect, points3d, mean_desc, desc2d, kpts2d, scores2d, kpt_offsets, image_hw, sample_image, sample_epoch,
                 descriptors2d_query, keypoints2d, keypoints3d, descriptors3d_db, descriptors2d_db);
    if (misaligned(collect, 16)) return fail(-1, "%s: collect must be 16-byte aligned", who);
    if (misaligned(kpts2d, 8)) return fail(-1, "%s: kpts2d must be 8-byte aligned", who);
    if (misaligned(scores_query, 4)) return fail(-1, "%s: a pointer is misaligned", who);
    const Layout L = make_layout(0, b, shape3d, num_leaf);
    if (int rc = check_workspace(who, workspace, workspace_bytes, L.total)) return rc;
    int32_t* leaf_src = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + L.leaf_src);
    hipStream_t st = as_stream(queue);
    if (int rc = launch_select(point_offsets, N, sample_image, sample_epoch, b, shape3d, num_leaf, seed, leaf_src, st)) return rc;
    if (int rc = launch_gather(collect, K, leaf_src, b, shape3d * num_leaf, descriptors2d_db, st)) return rc;
    if (int rc = launch_pad_query(desc2d, kpts2d, scores2d, kpt_offsets, image_hw, V, sample_image, sample_epoch, b, shape2d, seed,
                                  descriptors2d_query, keypoints2d, scores_query, st))
        return rc;
    return launch_pad_points(points3d, mean_desc, N, sample_image, sample_epoch, b, shape3d, seed, keypoints3d, descriptors3d_db, st);
}

}  // extern "C"
