// Shared host/device definitions: the column layout of the activation state in HBM, the
// workspace carve-up and the packed-weights blob.  See DESIGN.md "Data layout in HBM".
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "capi_common.h"

namespace gatsspg {

using capi::round_up;

constexpr int D = 256;    // descriptor_dim (hard-coded by the reference GNN, GATs_SuperGlue.py:35-36)
constexpr int H = 4;      // heads (GATs_SuperGlue.py:43)
constexpr int DH = 64;    // channels per head
constexpr int CP = 128;   // column padding granule: every (frame, side) segment starts on a multiple of CP
constexpr int BK = 32;    // K tile of every MFMA GEMM
constexpr int KVMAX = 8;           // bound data of a KV partial (message-operator scale of the fp16 modes): [0..3] per-wave largest key sum of the tile, [4..7] max |V| of the tile
constexpr int KVP = DH * DH + DH + KVMAX;  // one KV partial: the 64x64 KV matrix TRANSPOSED, [d][q] (kv_final owns 4-row d blocks), + 64 ksum + maxima
constexpr int MOP_LD = 512;        // row stride of the per-segment message operators M_seg [512][256] (two segments share a [512][512] block)
constexpr int MPL_PLANE = 512 * 256;   // bf16 elements of one split plane of M_seg (slab-major like the weight planes)

// tile widths baked into the partial-sum buffers
constexpr int QKV_BN = 64;    // column tile of the QKV+KV-partial kernel (one KV partial per tile)
constexpr int MLP0_BN = 64;   // column tile of the mlp.0 kernel (one InstanceNorm partial per tile)
constexpr int SC_BM = 128;    // score kernel row tile (over n1)
constexpr int SC_BN = 64;     // score kernel column tile (over n2)
constexpr int CF_ROWS = 16;   // conf-finalize strip height: 4 waves x 4 rows, all loaded before any is processed
constexpr int CF_COLS = 512;  // conf-finalize chunk width: 2 x 16 B per lane and row

// Activation state: channel-major [channels][ld] fp32; frame f owns columns [f*np, (f+1)*np):
// its N_2D query points at [0, n1) of that range (padded to n1p), its N_3D points at
// [n1p, n1p + n2) (padded to n2p).  A "segment" is one (frame, side) pair: seg = 2*f + side.
struct ColLayout {
    int b, n1, n2, n1p, n2p, np, ld;
    // active column window of a launch, per frame, in 64-column tiles: tiles [tw_first, tw_first + tw_count) of
    // every frame (default: the whole frame).  Lets the per-point kernels run on the query side or the 3D side only.
    int tw_first, tw_count;
    int side_mask;   // bit 0: 2D-side segments active, bit 1: 3D-side segments (segment-level reduction kernels)
    int xgs;         // XCD granule of the split kernels' tile map, log2 of column tiles (xcd_tile_map_g); always 0
    // nullptr, or a device word written earlier on the stream: while it reads 0 the launch does nothing (launch_is_off).  The plain
    // forward's database reuse points its prepare chain at the "database or weights changed" word of the comparison (db_verify_share).
    const int* gate;
};

__host__ __device__ inline ColLayout make_layout(int b, int n1, int n2) {
    ColLayout L;
    L.b = b; L.n1 = n1; L.n2 = n2;
    L.n1p = round_up(n1, CP); L.n2p = round_up(n2, CP);
    L.np = L.n1p + L.n2p; L.ld = b * L.np;
    L.tw_first = 0; L.tw_count = L.np / 64; L.side_mask = 3; L.xgs = 0; L.gate = nullptr;
    return L;
}
// first statement of every kernel that a gated chain launches (uniform over the grid: nobody reaches a barrier)
__device__ __forceinline__ bool launch_is_off(const ColLayout& L) { return L.gate != nullptr && *L.gate == 0; }

// layout restricted to one side: side 0 = query (2D) columns, 1 = 3D columns
__host__ __device__ inline ColLayout side_window(ColLayout L, int side) {
    L.tw_first = side ? L.n1p / 64 : 0;
    L.tw_count = (side ? L.n2p : L.n1p) / 64;
    L.side_mask = side ? 2 : 1;
    return L;
}
// number of active 64-column tiles of a launch, and the global tile index of active tile t
__host__ __device__ inline int active_tiles(const ColLayout& L) { return L.b * L.tw_count; }
__host__ __device__ inline int global_tile(const ColLayout& L, int t) {
    return (t / L.tw_count) * (L.np / 64) + L.tw_first + t % L.tw_count;
}

// Ragged frame batch against ONE shared database (gatsspg_forward_frames): the same column layout with n1 / n1p as the
// CAPACITY of every frame's query side -- addresses: segment starts, MDT rows, partial strides, the frame stride of conf -- and the
// frames' own query counts beside it, by value in the kernel arguments.  Every bound of a loop, mask, partition or tile count takes
// the frame's own count (q_n / q_np below): what the frame would see alone.  The database-side inputs (cache, leaves) are read with
// frame stride 0 (db_frame).  `skip`: frames a launch leaves out (bit f) -- a stage whose kernel form is chosen by the size of the
// frame ALONE runs once per form, each launch on the frames of its form.
// The kernels take the layout type as a template argument; on a ColLayout the accessors are the plain fields.
constexpr int MAX_FRAMES = 32;
struct FramesLayout : ColLayout {
    unsigned skip;
    int cnt[MAX_FRAMES];
};
template <class LT> inline constexpr bool is_frames = false;
template <> inline constexpr bool is_frames<FramesLayout> = true;
// frame f's own query count, and its padded count (what make_layout gives the frame alone)
__host__ __device__ inline int q_n(const ColLayout& L, int) { return L.n1; }
__host__ __device__ inline int q_n(const FramesLayout& L, int f) { return L.cnt[f]; }
__host__ __device__ inline int q_np(const ColLayout& L, int) { return L.n1p; }
__host__ __device__ inline int q_np(const FramesLayout& L, int f) { return round_up(L.cnt[f], CP); }
// frame index into the database-side inputs
__host__ __device__ inline int db_frame(const ColLayout&, int f) { return f; }
__host__ __device__ inline int db_frame(const FramesLayout&, int) { return 0; }
// a count of partials over the query rows of frame f (`per` rows each): the launch's own (capacity) count on a ColLayout
__host__ __device__ inline int q_parts(const ColLayout&, int, int, int launch_count) { return launch_count; }
__host__ __device__ inline int q_parts(const FramesLayout& L, int f, int per, int) { return (L.cnt[f] + per - 1) / per; }
// true for a column tile at c0 that the launch leaves alone: a skipped frame, or query-side columns past the frame's own padded count
__host__ __device__ inline bool tile_dead(const ColLayout&, int) { return false; }
__host__ __device__ inline bool tile_dead(const FramesLayout& L, int c0) {
    const int f = c0 / L.np, r = c0 - f * L.np;
    return ((L.skip >> f) & 1) || (r < L.n1p && r >= round_up(L.cnt[f], CP));
}

struct TileSeg {
    int frame, side, seg, seg_start, valid;  // valid = number of real (non-pad) columns in the tile
};

template <class LT>
__host__ __device__ inline TileSeg tile_seg(const LT& L, int c0, int bn) {
    TileSeg t;
    t.frame = c0 / L.np;
    int r = c0 - t.frame * L.np;
    t.side = r >= L.n1p ? 1 : 0;
    t.seg = t.frame * 2 + t.side;
    t.seg_start = t.frame * L.np + (t.side ? L.n1p : 0);
    int v = t.seg_start + (t.side ? L.n2 : q_n(L, t.frame)) - c0;
    t.valid = v < 0 ? 0 : (v > bn ? bn : v);
    return t;
}

// ---- packed weights blob (floats) -------------------------------------------------------------
struct AttnW {  // offsets inside one attention layer block
    static constexpr size_t WQKV = 0;                          // [768][256] rows: Q head-major, then per head K_h(64) V_h(64)
    static constexpr size_t BQKV = WQKV + 768 * 256;           // [768]
    static constexpr size_t W0 = BQKV + 768;                   // [512][512]: [:, :256] = mlp.0 x-half, [:, 256:] = W0b @ Wm (head-major cols)
    static constexpr size_t B0 = W0 + 512 * 512;               // [512] = b0 + W0b @ bm
    static constexpr size_t W3 = B0 + 512;                     // [256][512]
    static constexpr size_t B3 = W3 + 256 * 512;               // [256]
    // [8]: [0..2] the exact powers of two the fp16 planes of WQKV, W0[:, :256] and W3 are multiplied by before the split
    // (weight_scale_kernel: the matrix maximum lands in [2^13, 2^14)); [3] spare; [4 + h] = max_r sum_q |(W0b Wm)[r][h*64 + q]|, the
    // row-L1 norm of head h's message half: kv_final bounds the operator M_h with it.  The consumers scale the accumulators back.
    static constexpr size_t SC = B3 + 256;
    static constexpr size_t SIZE = SC + 8;
};
struct GatsW {
    static constexpr size_t U1 = 0;              // [256] = W @ a[:256]   (leaf logit vector)
    static constexpr size_t U2 = 256;            // [256] = W @ a[256:]   (3D-point logit vector)
    static constexpr size_t W = 512;             // [256][256] raw W (only used with_linear_transform)
    static constexpr size_t SIZE = 512 + 256 * 256;
};
constexpr size_t PW_ATTN = 0;
constexpr size_t PW_GATS = PW_ATTN + 8 * AttnW::SIZE;
constexpr size_t PW_FINAL_W = PW_GATS + 4 * GatsW::SIZE;
constexpr size_t PW_FINAL_B = PW_FINAL_W + 256 * 256;
constexpr size_t PW_TOTAL = PW_FINAL_B + 256;   // floats

// Split-bf16 planes of the three big GEMM operators (GATSSPG_FLAG_PREC_BF16X3 / _BF16X6): appended to the fp32 blob, in bf16
// elements from (unsigned short*)(packed + PW_TOTAL).  w = hi + lo with hi = RNE_bf16(w), lo = RNE_bf16(w - hi);
// rows in the order of the fp32 matrices they are split from, elements slab-major: (m, k) at ((k / 32) * M + m) * 32 + k % 32.
struct AttnWB {
    static constexpr size_t QKV_HI = 0;                          // [768][256]
    static constexpr size_t QKV_LO = QKV_HI + 768 * 256;
    static constexpr size_t W0_HI = QKV_LO + 768 * 256;          // [512][512]
    static constexpr size_t W0_LO = W0_HI + 512 * 512;
    static constexpr size_t W3_HI = W0_LO + 512 * 512;           // [256][512]
    static constexpr size_t W3_LO = W3_HI + 256 * 512;
    // third planes (GATSSPG_FLAG_PREC_BF16X6): lo2 = RNE_bf16(w - hi - lo), w = hi + lo + lo2 exactly
    static constexpr size_t QKV_LO2 = W3_LO + 256 * 512;
    static constexpr size_t W0_LO2 = QKV_LO2 + 768 * 256;
    static constexpr size_t W3_LO2 = W0_LO2 + 512 * 512;
    // fp16 hi / lo planes (GATSSPG_FLAG_PREC_FP16X3 / _FP16X4) of s * w, s = the matrix's power-of-two scale (AttnW::SC):
    // hi = RNE_fp16(s w), lo = RNE_fp16(s w - hi), same slab-major layout
    static constexpr size_t QKV_H16 = W3_LO2 + 256 * 512;
    static constexpr size_t QKV_L16 = QKV_H16 + 768 * 256;
    static constexpr size_t W0_H16 = QKV_L16 + 768 * 256;
    static constexpr size_t W0_L16 = W0_H16 + 512 * 512;
    static constexpr size_t W3_H16 = W0_L16 + 512 * 512;
    static constexpr size_t W3_L16 = W3_H16 + 256 * 512;
    static constexpr size_t SIZE = W3_L16 + 256 * 512;
};
constexpr size_t PWB_TOTAL = 8 * AttnWB::SIZE;                   // bf16 elements
constexpr size_t PACKED_BYTES = sizeof(float) * PW_TOTAL + sizeof(unsigned short) * PWB_TOTAL;

// Host-side views of one layer of the blob: what the launchers take instead of pointers into it.
struct WPlanes { const unsigned short *hi, *lo, *lo2, *h16, *l16; };   // the 16-bit planes of one operator
struct AttnLayer {
    const float* w;             // the layer's AttnW block
    const unsigned short* wb;   // the layer's AttnWB block
    const float* WQKV() const { return w + AttnW::WQKV; }
    const float* BQKV() const { return w + AttnW::BQKV; }
    const float* W0() const { return w + AttnW::W0; }
    const float* B0() const { return w + AttnW::B0; }
    const float* W3() const { return w + AttnW::W3; }
    const float* B3() const { return w + AttnW::B3; }
    const float* SC() const { return w + AttnW::SC; }
    WPlanes qkv_planes() const { return {wb + AttnWB::QKV_HI, wb + AttnWB::QKV_LO, wb + AttnWB::QKV_LO2, wb + AttnWB::QKV_H16, wb + AttnWB::QKV_L16}; }
    WPlanes w0_planes() const { return {wb + AttnWB::W0_HI, wb + AttnWB::W0_LO, wb + AttnWB::W0_LO2, wb + AttnWB::W0_H16, wb + AttnWB::W0_L16}; }
    WPlanes w3_planes() const { return {wb + AttnWB::W3_HI, wb + AttnWB::W3_LO, wb + AttnWB::W3_LO2, wb + AttnWB::W3_H16, wb + AttnWB::W3_L16}; }
};
struct GatsLayer {
    const float* w;             // the layer's GatsW block
    const float* U1() const { return w + GatsW::U1; }
    const float* U2() const { return w + GatsW::U2; }
    const float* W() const { return w + GatsW::W; }
};
inline AttnLayer attn_layer(const float* packed, int layer) {
    return {packed + PW_ATTN + (size_t)layer * AttnW::SIZE, reinterpret_cast<const unsigned short*>(packed + PW_TOTAL) + (size_t)layer * AttnWB::SIZE};
}
inline GatsLayer gats_layer(const float* packed, int layer) { return {packed + PW_GATS + (size_t)layer * GatsW::SIZE}; }

// The arithmetic of a call's qkv_kv / mlp0 / mlp3 main loops, from the GATSSPG_FLAG_PREC_* bit of its flags: exact fp32 MFMA, three- / six-term
// split-bf16, three- / four-term split-fp16.  The values are kernel and template arguments (PREC of the register-staged kernels: FP32..BF16X6;
// MODE of the split-loop tiles: BF16X6..FP16X4) and with that part of the kernel names: they do not change.
enum Arith : int { FP32 = 0, BF16X3 = 1, BF16X6 = 2, FP16X3 = 3, FP16X4 = 4 };
constexpr bool is_fp16(Arith a) { return a >= FP16X3; }                // also: the three GEMMs run on the split loop (gatsspg_split_kernels.hip)
constexpr bool needs_operator_planes(Arith a) { return a != FP32; }   // mlp0 multiplies 16-bit planes of the message operator (Workspace::Mpl), not Mop

// ---- database cache: everything of the first three GNN layers that depends only on the
//      per-object 3D database.  Layout (floats): Y2 [b][256][n2] | QY [b][256][n2] | kvY [b][4][KVP] |
//      LL [3][b][tiles][32] (leaf logits of GATs layers 1..3; layer 0 is inside Y2)
struct DbCache {
    float *Y2, *QY, *kvY, *LL;
    size_t ll_layer;   // floats per layer of LL
    size_t bytes;
};
size_t gats_leaf_logit_floats(int b, int n2);   // gatsspg_stream_kernels.hip
inline DbCache carve_cache(void* base, int b, int n2) {
    DbCache c;
    capi::Bump a(base, sizeof(float));   // packed: the layout is part of the ABI (gatsspg_version)
    const size_t plane = sizeof(float) * (size_t)b * D * n2;
    c.Y2 = a.take<float>(plane);
    c.QY = a.take<float>(plane);
    c.kvY = a.take<float>(sizeof(float) * (size_t)b * H * KVP);
    c.ll_layer = gats_leaf_logit_floats(b, n2);
    c.LL = a.take<float>(sizeof(float) * 3 * c.ll_layer);
    c.bytes = a.off;
    return c;
}

// ---- reuse area of the plain forward (gatsspg_forward): the last piece of a workspace, state that one call leaves for
//      the next.  A DbCache of the database the workspace saw last, a bitwise snapshot of that database and of the packed-weight
//      ranges the cache depends on (GATs layer 0, attention layers 0 and 1), a second copy of the cache, and the words below.
//      Every call compares the caller's tensors with the snapshot and the cache with its copy, word for word (db_verify_share: as extra
//      workgroups of the call's first GEMM launches, which touch query columns only, or as the db_verify_kernel launch behind them); only a
//      call that finds them all equal reads the cache.  Order: cache | snapshot pieces 0..6 | cache copy | state.
constexpr int REUSE_MAGIC = 0x67447265;
struct ReuseStamp { int magic, b, n1p, n2, num_leaf, flags; };   // what a snapshot was taken under; n1p: the area's offset and the kernel forms go by it
struct ReuseState {
    ReuseStamp stamp;
    unsigned fingerprint;   // of the previous call's database (a sum over a strided sample): decides whether a snapshot is worth taking, never a hit
    int snapshot_valid;     // 1: snapshot and cache are those of one database, taken under `stamp`
    int miss;               // this call: OR-ed to 1 by every mismatch the comparison finds; the gate of the prepare chain; db_settle_kernel
                            // clears it again and leaves the verdict in `hit` (a word of garbage here costs one miss)
    int strike;             // this call: its fingerprint is the previous call's (same stamp)
    int hit;                // this call's outcome, for the caller to read back: 1 = the cache was reused
    int copy;               // this call: db_snapshot_kernel copies (a miss with a strike)
    int spare[4];
};
static_assert(sizeof(ReuseState) == 64, "the state block is sixteen words");
// the compared / snapshotted tensors: piece p is n[p] 16-byte words
// 0 desc3d_db, 1 desc2d_db, 2 GATs layer 0, 3 / 4 attention layers 0 / 1 (fp32 blocks), 5 / 6 their 16-bit planes (split arithmetics only),
// 7 the cache itself (Y2 | QY | kvY) against a second copy: a call of another shape on the same memory may have written into it
constexpr int DB_PIECES = 8;
struct DbPieces {
    const uint4* cur[DB_PIECES];
    uint4* snap[DB_PIECES];
    unsigned long long n[DB_PIECES];
};
struct ReuseArea {
    bool present;        // false: this shape never takes the reusing path (db_reuse_shape), the workspace has no area
    DbCache cache;
    char* snap[DB_PIECES];
    ReuseState* state;   // the last piece: at gatsspg_workspace_bytes(...) - 256 (include/gatsspg.h tells callers so)
};
inline size_t db_piece_bytes(int p, int b, int n2, int num_leaf) {
    static_assert((GatsW::SIZE * sizeof(float)) % 16 == 0 && (AttnW::SIZE * sizeof(float)) % 16 == 0 && (AttnWB::SIZE * sizeof(unsigned short)) % 16 == 0 &&
                      (PW_GATS * sizeof(float)) % 16 == 0 && (PW_TOTAL * sizeof(float)) % 16 == 0,
                  "every compared weight range is a whole number of 16-byte words of a 16-byte aligned blob");
    const size_t plane = sizeof(float) * (size_t)b * D * n2;   // D = 256: a multiple of 16 bytes for every b, n2
    static_assert((H * KVP * sizeof(float)) % 16 == 0, "so is the cache up to its leaf-logit table");
    return p == 0 ? plane : p == 1 ? plane * num_leaf : p == 2 ? sizeof(float) * GatsW::SIZE : p < 5 ? sizeof(float) * AttnW::SIZE
         : p < 7 ? sizeof(unsigned short) * AttnWB::SIZE : 2 * plane + sizeof(float) * (size_t)b * H * KVP;
}
// Where gatsspg_forward takes the reusing path, by shape (gatsspg_gemm_kernels.hip, next to the launch thresholds it goes by)
bool db_reuse_shape(int b, int n1, int n2);

// The comparison rides on the three GEMM launches of attention layer 0 on the query window -- qkv_kv, mlp0, mlp3, the first launches of a
// reusing forward, which read neither cache nor database and leave most of the machine idle: extra workgroups behind the GEMM
// grid of each compare that launch's share of every piece.  Shares in proportion to the launches' measured times at the headline shape
// (16-tile query window: 13.9 / 21.3 / 19.5 us).  DB_RIDER_BLOCKS: rider workgroups per launch (of the GEMM kernel's 512 threads each);
// both from the sweep in DESIGN 10d, which is flat around these values.
constexpr int DB_RIDER_LAUNCHES = 3;
constexpr int DB_RIDER_WEIGHT[DB_RIDER_LAUNCHES] = {14, 21, 19};
constexpr int DB_RIDER_BLOCKS[DB_RIDER_LAUNCHES] = {128, 128, 128};
// words [*lo, *hi) of a piece of n 16-byte words that riding launch k compares: the shares tile [0, n) in order, without gap or overlap
inline void db_rider_share(unsigned long long n, int k, unsigned long long* lo, unsigned long long* hi) {
    unsigned long long before = 0, total = 0;
    for (int i = 0; i < DB_RIDER_LAUNCHES; ++i) {
        total += DB_RIDER_WEIGHT[i];
        if (i < k) before += DB_RIDER_WEIGHT[i];
    }
    *lo = n * before / total;                          // (n < 2^58: the products stay inside 64 bits)
    *hi = n * (before + DB_RIDER_WEIGHT[k]) / total;   // k = last: n * total / total = n
}
// What a launch that carries the comparison takes: the pieces, its share of each, and what the owner -- rider workgroup 0 of the first
// riding launch of a call (`owner`), or workgroup 0 of the stand-alone db_verify_kernel -- needs for the stamp and the fingerprint.
struct DbRider {
    DbPieces P;
    unsigned long long lo[DB_PIECES], hi[DB_PIECES];   // this launch compares words [lo, hi) of piece p
    ReuseState* st;
    int first_block, blocks;   // workgroups [first_block, first_block + blocks) of the grid are the riders
    int owner;
    ReuseStamp stamp;
    const unsigned *d3, *d2db;      // the database tensors as 4-byte words (fingerprint), n3 / n2 of them
    unsigned long long n3, n2;
};
// the layout of a GEMM launch that carries riders: the kernels take the role from the type (is_rider), so that only the riding launches
// instantiate it and the whole-frame kernels stay what they are
struct RiderLayout : ColLayout {
    DbRider rider;
};
template <class LT> inline constexpr bool is_rider = false;
template <> inline constexpr bool is_rider<RiderLayout> = true;

#if defined(__HIPCC__)
constexpr int DBV_UNROLL = 4;      // 4 x 2 independent 16-byte loads per thread and trip
constexpr int DBV_SAMPLES = 1024;  // fingerprint: this many 4-byte words of each database tensor (8 KB in all)
// words [lo + first, end) of one piece, every stride-th batch: the OR of all differences this thread saw
__device__ __forceinline__ unsigned db_compare_words(const uint4* __restrict__ cur, const uint4* __restrict__ snap, unsigned long long lo,
                                                     unsigned long long end, unsigned long long first, unsigned long long stride) {
    unsigned diff = 0;
    for (unsigned long long i0 = lo + first; i0 < end; i0 += stride * DBV_UNROLL) {
        uint4 a[DBV_UNROLL], c[DBV_UNROLL];
#pragma unroll
        for (int j = 0; j < DBV_UNROLL; ++j) {
            const unsigned long long i = i0 + j * stride;
            a[j] = c[j] = make_uint4(0, 0, 0, 0);
            if (i < end) {
                a[j] = cur[i];
                c[j] = snap[i];
            }
        }
#pragma unroll
        for (int j = 0; j < DBV_UNROLL; ++j) diff |= (a[j].x ^ c[j].x) | (a[j].y ^ c[j].y) | (a[j].z ^ c[j].z) | (a[j].w ^ c[j].w);
    }
    return diff;
}
// The comparison of one workgroup (`rider` of r.blocks, any block size) with its owner duties: every 16-byte word of its launch's share of
// every piece against the snapshot, as integers; one plain atomicOr per wave that saw a difference, none once the word is set.
// Nothing waits: the first reader of st->miss is a later launch on the stream.  The owner also checks stamp and snapshot_valid, computes
// the fingerprint, compares it with the stored one (strike) and stores fingerprint and stamp: exactly once per call.
__device__ __forceinline__ void db_verify_share(const DbRider& r, int rider) {
    ReuseState* st = r.st;
    const bool owner = r.owner && rider == 0;
    int same_stamp = 0;   // (thread 0 of the owner)
    if (owner && threadIdx.x == 0) {
        // a snapshot that is not valid, or was taken under another stamp, is a miss before anything is compared
        const ReuseStamp o = st->stamp, n = r.stamp;
        same_stamp = o.magic == n.magic && o.b == n.b && o.n1p == n.n1p && o.n2 == n.n2 && o.num_leaf == n.num_leaf && o.flags == n.flags;
        if (!same_stamp || st->snapshot_valid != 1) {
            st->snapshot_valid = 0;
            atomicOr(&st->miss, 1);
        }
    }
    // A word that already reads non-zero cannot change the outcome any more: the workgroups that start after the first difference was
    // recorded skip their share (a miss costs a fraction of the pass), and no wave adds an atomic to a word that is set (when nearly
    // every wave differs -- no valid snapshot -- 28 k atomics on one address took 200 us).  Which workgroups skip depends on their order;
    // whether the word ends non-zero does not.
    const bool skip = __hip_atomic_load(&st->miss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    const unsigned long long stride = (unsigned long long)r.blocks * blockDim.x, first = (unsigned long long)rider * blockDim.x + threadIdx.x;
    unsigned diff = 0;
#pragma unroll 1   // (a real loop: unrolled, the 8 x 4 piece arguments live at once spill scalar registers in the GEMM kernels)
    for (int p = 0; p < DB_PIECES; ++p) diff |= db_compare_words(r.P.cur[p], r.P.snap[p], r.lo[p], skip ? 0ull : r.hi[p], first, stride);
    // one plain atomic per wave that saw a difference: the word's value does not depend on who comes first
    if (__any(diff != 0) && (threadIdx.x & 63) == 0 && !__hip_atomic_load(&st->miss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&st->miss, 1);
    if (!owner) return;
    // fingerprint of this call's database, and the new stamp
    __shared__ unsigned fp;
    if (threadIdx.x == 0) fp = 0;
    __syncthreads();
    unsigned h = 0;
    for (int k = threadIdx.x; k < DBV_SAMPLES; k += blockDim.x)   // word k * n / SAMPLES of each tensor, weighted by its (odd) position
        h += r.d3[(unsigned long long)k * r.n3 / DBV_SAMPLES] * (2u * k + 1u) + r.d2db[(unsigned long long)k * r.n2 / DBV_SAMPLES] * (2u * (k + DBV_SAMPLES) + 1u);
    atomicAdd(&fp, h);   // (integer sum: the same value in every order)
    __syncthreads();
    if (threadIdx.x == 0) {
        st->strike = same_stamp && st->fingerprint == fp ? 1 : 0;
        st->fingerprint = fp;
        st->stamp = r.stamp;
    }
}
#endif

// ---- workspace carve-up ---------------------------------------------------------------------------
struct Workspace {
    ColLayout L;
    Arith prec;        // from the call's flags
    int nt64;          // ld / 64 column tiles
    int nseg;          // 2*b
    int sc_nct, sc_nrt;   // score kernel tiles per frame (n2p/SC_BN, n1p/SC_BM)
    int cf_nst, cf_nch;   // conf-finalize strips / chunks per frame
    float *Z, *Q, *MSG, *U, *MD;     // MD aliases Q (Q is dead after the GNN); MSG: scratch of the with_linear_transform GATs path
    float *MDT;                      // query-side normalised descriptors, point-major [b][n1p][256]; aliases MSG
    unsigned short *MDTp;            // their 16-bit planes for the split score contraction (bf16x6 / fp16x4): [3][8 slabs][b * n1p][32], slab-major
    float *kvpart, *kvfin, *statpart, *stats;
    int *statcnt;                    // [nseg][8] arrival counters of the fused InstanceNorm statistics (stat_last_block)
    // linear attention folded into mlp.0 (kv_final_kernel -> mlp0_kernel): per TARGET segment t the operator
    // M_t = (W0b Wm)[:, head h] KV_h(source) for the four heads [512][4 x 64], and the source's ksum.
    float *Mop;                      // [b][512][512]: segment 2f at columns 256..511, segment 2f+1 at columns 0..255 of frame f's block
    unsigned short *Mpl;             // 16-bit planes of M_t (needs_operator_planes): [nseg][3][8 slabs][512][32]
    float *ksumT;                    // [nseg][4][64]
    float *zsc;                      // [nseg][4]: per head, fold factor of the target segment's operator planes = (scale of the W0 planes) / (scale of Mpl_h), a power of two
    float *rowpart, *colpart, *rs, *cs;
    float *rmax_v, *cmax_v, *rshift, *cshift;   // rshift / cshift: row / column maxima of the max-subtracting dual softmax
    int *rmax_i, *cmax_i;
    size_t bytes;
    // ragged frame batch (gatsspg_forward_frames): the frames' own query counts; L then holds the capacity.  Host side only: a launcher
    // hands its kernel frames_layout(w) instead of w.L.
    bool frames;
    unsigned skip;             // frames the next launch leaves out (FramesLayout::skip)
    bool shared_leaf;          // GATs layers (num_leaf == 8, no linear transform) on the shared-leaf kernel: each leaf tile read once per group of frames
    int fcnt[MAX_FRAMES];
    // 0, or the 64-column tiles of the WHOLE frame this windowed launch is a part of: launch_by_form then goes by them, so that a one-side
    // window takes the kernel form the plain forward's whole-frame launch takes (the reusing path of gatsspg_forward: bit-identical to it)
    int form_tiles;
    // nullptr, or the DB_RIDER_LAUNCHES rider arguments of a reusing forward's part A (host side only): the fp32 qkv_kv / mlp0 / mlp3
    // launchers then take the riding instantiation with rider[0 / 1 / 2] (rider_layout)
    const DbRider* rider;
    ReuseArea R;
};
// the layout a riding launch hands its kernel: rider k of the call, behind a GEMM grid of `grid` workgroups
inline RiderLayout rider_layout(const Workspace& w, int k, int grid) {
    RiderLayout R;
    static_cast<ColLayout&>(R) = w.L;
    R.rider = w.rider[k];
    R.rider.first_block = grid;
    return R;
}
inline FramesLayout frames_layout(const Workspace& w) {
    FramesLayout F;
    static_cast<ColLayout&>(F) = w.L;
    F.skip = w.skip;
    for (int i = 0; i < MAX_FRAMES; ++i) F.cnt[i] = i < w.L.b ? w.fcnt[i] : 0;
    return F;
}
// calls f with the layout a kernel of this launch takes: w.L, or the frames layout
template <class F>
inline void with_layout(const Workspace& w, F&& f) {
    if (w.frames) f(frames_layout(w));
    else f(w.L);
}
inline unsigned all_frames(const Workspace& w) { return w.L.b >= 32 ? ~0u : (1u << w.L.b) - 1u; }
// 64-column tiles the launch window holds of frame f ALONE (what active_tiles is at b = 1): the figure the shape thresholds between two
// kernel forms go by
inline int alone_tiles(const Workspace& w, int f) {
    const int n1p = w.frames ? round_up(w.fcnt[f], CP) : w.L.n1p;
    return ((w.L.side_mask & 1) ? n1p / 64 : 0) + ((w.L.side_mask & 2) ? w.L.n2p / 64 : 0);
}
// A stage with two kernel forms chosen by a shape threshold `first(tiles)`: one launch as ever on a uniform layout; on a frames layout
// every frame takes the form it would take alone, so the stage is up to two launches, each skipping the other form's frames.
template <class Pred, class FA, class FB>
inline void launch_by_form(const Workspace& w, Pred first, FA fa, FB fb) {
    if (!w.frames) {
        if (first(w.form_tiles ? w.form_tiles : active_tiles(w.L))) fa(w);
        else fb(w);
        return;
    }
    unsigned ma = 0;
    for (int f = 0; f < w.L.b; ++f)
        if (first(alone_tiles(w, f))) ma |= 1u << f;
    const unsigned mb = all_frames(w) & ~ma;
    Workspace v = w;
    if (ma) { v.skip = w.skip | mb; fa(v); }
    if (mb) { v.skip = w.skip | ma; fb(v); }
}

// M_t of segment `seg`: element (r, c), c = h*64 + d, at mop_seg(Mop, seg)[r * MOP_LD + c]
__host__ __device__ inline float* mop_seg(float* Mop, int seg) { return Mop + (size_t)(seg >> 1) * 512 * MOP_LD + ((seg & 1) ? 0 : 256); }
__host__ __device__ inline const float* mop_seg(const float* Mop, int seg) {
    return Mop + (size_t)(seg >> 1) * 512 * MOP_LD + ((seg & 1) ? 0 : 256);
}

// num_leaf: 0 = without the reuse area (the pieces in front of it do not depend on num_leaf)
inline Workspace carve_workspace(void* base, int b, int n1, int n2, int num_leaf = 0) {
    Workspace w;
    w.form_tiles = 0;
    w.rider = nullptr;
    w.L = make_layout(b, n1, n2);
    w.prec = FP32;
    w.frames = false; w.skip = 0; w.shared_leaf = false;
    const ColLayout& L = w.L;
    w.nt64 = L.ld / 64;
    w.nseg = 2 * b;
    w.sc_nct = L.n2p / SC_BN;
    w.sc_nrt = L.n1p / SC_BM;
    w.cf_nst = (n1 + CF_ROWS - 1) / CF_ROWS;
    w.cf_nch = (n2 + CF_COLS - 1) / CF_COLS;
    capi::Bump a(base);
    const size_t ld = L.ld;
    w.Z = a.take<float>(sizeof(float) * D * ld);
    w.Q = a.take<float>(sizeof(float) * D * ld);
    w.MSG = a.take<float>(sizeof(float) * D * ld);
    w.U = a.take<float>(sizeof(float) * 2 * D * ld);
    w.MD = w.Q;
    w.MDT = w.MSG;   // b * n1p * 256 floats <= 256 * ld
    w.MDTp = a.take<unsigned short>(sizeof(unsigned short) * 3 * (size_t)b * L.n1p * D);
    w.kvpart = a.take<float>(sizeof(float) * (size_t)w.nt64 * H * KVP);
    w.kvfin = a.take<float>(sizeof(float) * (size_t)w.nseg * H * KVP);
    w.Mop = a.take<float>(sizeof(float) * (size_t)b * 512 * MOP_LD);
    w.Mpl = a.take<unsigned short>(sizeof(unsigned short) * (size_t)w.nseg * 3 * MPL_PLANE);
    w.ksumT = a.take<float>(sizeof(float) * (size_t)w.nseg * H * DH);
    w.zsc = a.take<float>(sizeof(float) * (size_t)w.nseg * H);
    w.statpart = a.take<float>(sizeof(float) * (size_t)w.nt64 * 2 * 2 * 512);   // one partial per 64 columns, or per 32 (mlp0_sp's transposed epilogue)
    w.stats = a.take<float>(sizeof(float) * (size_t)w.nseg * 2 * 512);
    w.statcnt = a.take<int>(sizeof(int) * (size_t)w.nseg * 8);
    w.rowpart = a.take<float>(sizeof(float) * (size_t)b * w.sc_nct * L.n1p);
    w.colpart = a.take<float>(sizeof(float) * (size_t)b * w.sc_nrt * L.n2p);
    w.rs = a.take<float>(sizeof(float) * (size_t)b * L.n1p);
    w.cs = a.take<float>(sizeof(float) * (size_t)b * L.n2p);
    w.rmax_v = a.take<float>(sizeof(float) * (size_t)b * w.cf_nch * L.n1p);
    w.rmax_i = a.take<int>(sizeof(int) * (size_t)b * w.cf_nch * L.n1p);
    w.cmax_v = a.take<float>(sizeof(float) * (size_t)b * w.cf_nst * L.n2p);
    w.cmax_i = a.take<int>(sizeof(int) * (size_t)b * w.cf_nst * L.n2p);
    w.rshift = a.take<float>(sizeof(float) * (size_t)b * L.n1p);
    w.cshift = a.take<float>(sizeof(float) * (size_t)b * L.n2p);
    // the reuse area: behind everything else, so that no other offset moves
    w.R.present = num_leaf > 0 && db_reuse_shape(b, n1, n2);
    if (w.R.present) {
        w.R.cache = carve_cache(a.take<char>(carve_cache(nullptr, b, n2).bytes), b, n2);
        for (int p = 0; p < DB_PIECES; ++p) w.R.snap[p] = a.take<char>(db_piece_bytes(p, b, n2, num_leaf));
        static_assert(sizeof(ReuseState) <= 256, "one allocation granule");
        w.R.state = a.take<ReuseState>(sizeof(ReuseState));
    }
    w.bytes = a.off;
    return w;
}

}  // namespace gatsspg
