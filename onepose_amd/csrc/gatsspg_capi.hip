// C ABI of libgatsspg_hip.so (declared in include/gatsspg.h).  Thin: argument checks, workspace
// carve-up, kernel enqueue on the caller's stream.  No allocation, no synchronisation.

#include "../../include/gatsspg.h"
#include "gatsspg_launch.h"

using namespace gatsspg;
using namespace capi;

namespace {
int check_dims(int b, int n1, int n2, int num_leaf) {
    if (b < 1) return fail(1, "batch must be >= 1 (got %d)", b);
    // the reference returns early for an empty side (GATs_SuperGlue.py:195) and InstanceNorm1d raises for
    // a single point (:126); both are handled by the host-side module, never enqueued.
    if (n1 < 2 || n2 < 2) return fail(1, "n1 and n2 must be >= 2 (got n1=%d n2=%d)", n1, n2);
    if (num_leaf < 1 || num_leaf > 64) return fail(1, "num_leaf must be in [1, 64] (got %d)", num_leaf);
    const long long ld = (long long)b * (round_up(n1, CP) + round_up(n2, CP));
    if (ld * 512 >= (1ll << 31)) return fail(1, "problem too large: b*(n1p+n2p) = %lld columns", ld);
    if ((long long)n1 * n2 >= (1ll << 31)) return fail(1, "n1*n2 too large");
    return 0;
}

// the one place where the ABI's flag bits become an Arith
int arith_of_flags(int flags, Arith& a) {
    constexpr int PREC_BITS = GATSSPG_FLAG_PREC_BF16X3 | GATSSPG_FLAG_PREC_BF16X6 | GATSSPG_FLAG_PREC_FP16X3 | GATSSPG_FLAG_PREC_FP16X4;
    if (flags & ~(GATSSPG_FLAG_INCLUDE_SELF | GATSSPG_FLAG_ADDITIONAL | GATSSPG_FLAG_WITH_LINEAR_TRANSFORM | PREC_BITS | GATSSPG_FLAG_NO_DB_REUSE))
        return fail(1, "unknown bits in flags (0x%x)", flags);
    constexpr int BIT[] = {0, GATSSPG_FLAG_PREC_BF16X3, GATSSPG_FLAG_PREC_BF16X6, GATSSPG_FLAG_PREC_FP16X3, GATSSPG_FLAG_PREC_FP16X4};   // by Arith
    for (int i = FP32; i <= FP16X4; ++i)
        if ((flags & PREC_BITS) == BIT[i]) { a = Arith(i); return 0; }
    return fail(1, "GATSSPG_FLAG_PREC_BF16X3, _BF16X6, _FP16X3 and _FP16X4 are exclusive");
}

int check_ws(const void* ws, size_t ws_bytes, int b, int n1, int n2, int num_leaf, Workspace& w, int flags = 0) {
    if (int e = check_dims(b, n1, n2, num_leaf)) return e;
    if (!ws) return fail(1, "workspace pointer is null");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(1, "workspace must be 16-byte aligned");
    w = carve_workspace(const_cast<void*>(ws), b, n1, n2, num_leaf);
    if (int e = arith_of_flags(flags, w.prec)) return e;
    if (ws_bytes < w.bytes) return fail(1, "workspace too small: %zu < %zu bytes", ws_bytes, w.bytes);
    return 0;
}

// The dual softmax is evaluated without max-subtraction whenever that is safe: the scores are cosines / scale_factor, so
// exp() stays in range as long as 1 / scale_factor <= 80 (exp(80) = 5.5e34, row sums of 1e5 terms still fit fp32; the
// reference's 0.07 gives 14.3) and one pass over S yields both normalisers.  Smaller scale factors take the
// max-subtracting path (raw scores -> row/column maxima and shifted sums -> finalize), which has the full range of
// torch.softmax (GATs_SuperGlue.py:218).
int check_scale(float scale_factor) { return scale_factor > 0.f ? 0 : fail(1, "scale_factor must be positive"); }
inline int softmax_shifted(float scale_factor) { return scale_factor < 0.0125f ? 1 : 0; }

// h3 / dq: fused state load (see launch_gats); only valid when gats_fuses_state_load() says so
void enqueue_gats(const float* packed, int layer, const float* desc2d_db, int num_leaf, int flags, const Workspace& w,
                  hipStream_t s, ProfileHook* hk = nullptr, const float* h3 = nullptr, const float* dq = nullptr,
                  const float* cached_logits = nullptr) {
    const GatsLayer g = gats_layer(packed, layer);
    if (flags & GATSSPG_FLAG_WITH_LINEAR_TRANSFORM) {
        // pre-activation aggregate -> MSG (free between attention layers), then elu(W^T pre (+h))
        launch_gats(g, desc2d_db, num_leaf, flags, w.MSG, w, s, hk);
        const int add_h = (flags & GATSSPG_FLAG_INCLUDE_SELF) && (flags & GATSSPG_FLAG_ADDITIONAL);
        launch_gats_wlt(g, w.MSG, w, add_h, s, hk);
    } else {
        launch_gats(g, desc2d_db, num_leaf, flags, w.Z, w, s, hk, h3, dq, cached_logits);
    }
}

void enqueue_attn(const float* packed, int layer, int kind, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr) {
    const AttnLayer a = attn_layer(packed, layer);
    launch_qkv_kv(a, w, s, hk);
    launch_kv_final(a, w, kind == GATSSPG_LAYER_CROSS, nullptr, s, hk);
    launch_mlp(a, w, s, hk);
}

// rounds t0..3 of ['GATs', 'self', 'cross'] (GATs_SuperGlue.py:162).  h3 / dq: the fused state load of round 0 (enqueue_gats), or null;
// ll: the cached leaf logits of rounds 1..3, ll_layer floats apart (DbCache::LL), or null
void enqueue_rounds(const float* packed, int t0, const float* desc2d_db, int num_leaf, int flags, const Workspace& w, hipStream_t s,
                    ProfileHook* hk, const float* h3, const float* dq, const float* ll, size_t ll_layer) {
    for (int t = t0; t < 4; ++t) {
        enqueue_gats(packed, t, desc2d_db, num_leaf, flags, w, s, hk, t ? nullptr : h3, t ? nullptr : dq, t && ll ? ll + (size_t)(t - 1) * ll_layer : nullptr);
        enqueue_attn(packed, 2 * t, GATSSPG_LAYER_SELF, w, s, hk);
        enqueue_attn(packed, 2 * t + 1, GATSSPG_LAYER_CROSS, w, s, hk);
    }
}

// final projection (packed == nullptr: already done, w.MD / w.MDT hold the descriptors), score, dual softmax and match
void enqueue_tail(const float* packed, const Workspace& w, float scale_factor, float match_threshold, const MatchOut& out, hipStream_t s, ProfileHook* hk) {
    const int shifted = softmax_shifted(scale_factor);
    if (packed) launch_final_proj_norm(packed + PW_FINAL_W, packed + PW_FINAL_B, w, s, hk);
    launch_score_exp(w, out.conf, scale_factor, shifted, s, hk);
    launch_dual_softmax_match(w, out, shifted, match_threshold, s, hk);
}
int check_out(const MatchOut& o) { return o.conf && o.matches0 && o.matches1 && o.mscores0 && o.mscores1 ? 0 : fail(1, "null output pointer"); }

Workspace windowed(const Workspace& w, int side) {
    Workspace v = w;
    v.L = side_window(w.L, side);
    return v;
}

// The prepare chain: everything of the first three GNN layers that depends on the database and the weights alone, into the cache `c`.
// w: a workspace carved with 2 dummy (zero) query columns (gatsspg_prepare_database), or -- with `settle` -- the workspace of a reusing
// forward itself: the chain then runs on the 3D-side columns of the call's own layout and leaves alone what the call's part A wrote (query
// columns of state and Q, their KV partials; the per-segment sums, statistics and operators of the query side it does overwrite are
// consumed by then or written again by part B).  Every launch takes w.L.gate (the reusing path of gatsspg_forward: the chain does nothing
// while the gate word reads 0).  ll: also the leaf logits of the three GATs layers still to come (DbCache::LL).
// settle: the reusing path's state block, whose verdict the last launch then settles (launch_db_settle), or null.
void enqueue_prepare(const float* packed, const float* desc3d_db, const float* desc2d_db, int num_leaf, int flags, const Workspace& w,
                     const DbCache& c, bool ll, ReuseState* settle, hipStream_t s) {
    const Workspace wy = windowed(w, 1);
    if (settle) launch_load_columns(nullptr, desc3d_db, w.Z, w, s);         // the query columns stay
    else launch_load_state(nullptr, desc3d_db, w, s);
    enqueue_gats(packed, 0, desc2d_db, num_leaf, flags, w, s);              // gnn.layers.0 (3D side only by nature)
    enqueue_attn(packed, 0, GATSSPG_LAYER_SELF, wy, s);                     // gnn.layers.1, 3D side
    const AttnLayer a1 = attn_layer(packed, 1);
    launch_qkv_kv(a1, wy, s);                                               // gnn.layers.2: 3D-side Q, KV, ksum
    launch_kv_final(a1, wy, 1, nullptr, s);                                 //   (the final sums land in w.kvfin)
    launch_store_state(w.Z, nullptr, c.Y2, w, s);
    launch_store_state(w.Q, nullptr, c.QY, w, s);
    if (settle) launch_db_settle(c.kvY, w, settle, s);
    else launch_store_kv_sums(c.kvY, w, s);
    if (ll) launch_gats_leaf_logits(gats_layer(packed, 1), 3, desc2d_db, c.LL, w, s);   // leaf . u1 of the three GATs layers still to come
}

// The cached chain: the forward from a cache of the prepare chain, in two halves split at the first use of the cache.
// w: the call's workspace, or its frames form (gatsspg_forward_frames).
// Part A, the query side: nothing here reads the cache, the database or (reusing path) the verdict.  With w.rider the three GEMM launches
// of gnn.layers.1 carry the database comparison.  (The projection of gnn.layers.2 as a fourth riding launch: no difference)
void enqueue_cached_query(const float* packed, const float* desc2d_query, const Workspace& w, hipStream_t s) {
    Workspace wx = windowed(w, 0);
    launch_load_columns(desc2d_query, nullptr, w.Z, w, s);                  // state = [X0 (of every frame) | ...]
    enqueue_attn(packed, 0, GATSSPG_LAYER_SELF, wx, s);                     // gnn.layers.1, query side only
    wx.rider = nullptr;
    launch_qkv_kv(attn_layer(packed, 1), wx, s);                            // gnn.layers.2: query-side Q, KV, ksum
}
// Part B: everything from the cache on.
void enqueue_cached_rest(const float* packed, const float* desc2d_db, const DbCache& c, bool ll, int num_leaf, int flags, float scale_factor,
                         float match_threshold, const MatchOut& out, const Workspace& w, hipStream_t s) {
    const AttnLayer a1 = attn_layer(packed, 1);
    launch_load_db_columns(c.Y2, w.Z, c.QY, w.Q, w, s);                     // state = [... | cached Y2], 3D-side Q from the cache
    launch_kv_final(a1, w, 1, c.kvY, s);                                    // query-side sums from the partials, 3D-side sums from the cache
    launch_mlp(a1, w, s);
    enqueue_rounds(packed, 1, desc2d_db, num_leaf, flags, w, s, nullptr, nullptr, nullptr, ll ? c.LL : nullptr, c.ll_layer);
    enqueue_tail(packed, w, scale_factor, match_threshold, out, s, nullptr);
}
void enqueue_cached(const float* packed, const float* desc2d_query, const float* desc2d_db, const DbCache& c, bool ll, int num_leaf, int flags,
                    float scale_factor, float match_threshold, const MatchOut& out, const Workspace& w, hipStream_t s) {
    enqueue_cached_query(packed, desc2d_query, w, s);
    enqueue_cached_rest(packed, desc2d_db, c, ll, num_leaf, flags, scale_factor, match_threshold, out, w, s);
}

// The tensors the comparison reads and db_snapshot_kernel copies: the database, and the packed-weight ranges the cache is computed
// from -- GATs layer 0, attention layers 0 and 1; their 16-bit planes only under the arithmetics that read them -- and the cache against its copy.
DbPieces db_pieces(const float* packed, const float* desc3d_db, const float* desc2d_db, const Workspace& w, int num_leaf) {
    const AttnLayer a0 = attn_layer(packed, 0), a1 = attn_layer(packed, 1);
    const void* cur[DB_PIECES] = {desc3d_db, desc2d_db, gats_layer(packed, 0).w, a0.w, a1.w, a0.wb, a1.wb, w.R.cache.Y2};
    DbPieces P;
    for (int p = 0; p < DB_PIECES; ++p) {
        P.cur[p] = static_cast<const uint4*>(cur[p]);
        P.snap[p] = reinterpret_cast<uint4*>(w.R.snap[p]);
        P.n[p] = (p == 5 || p == 6) && w.prec == FP32 ? 0 : db_piece_bytes(p, w.L.b, w.L.n2, num_leaf) / 16;
    }
    return P;
}

// The plain forward on a shape of db_reuse_shape: ONE fixed sequence of launches, the device chooses which of them work.
//   1. Part A of the cached chain, the query side.  Its three GEMM launches of gnn.layers.1 carry the comparison of the caller's database
//      and weights with the workspace's snapshot, word for word, as extra workgroups (db_rider_share decides which launch compares which
//      words of which piece; rider 0 of the first launch owns stamp and fingerprint).  A frame whose part A does not take the riding
//      instantiations (the split arithmetics, a query window of more than DIET_MIN_TILES tiles) runs the same comparison as one launch behind A.
//   2. The prepare chain on the 3D-side columns of the same layout, gated on the verdict (a hit: a dozen empty launches; a miss: the cache
//      is rebuilt from this call's inputs, what part A wrote stays); its last launch settles the verdict.
//   3. db_snapshot keeps the inputs for the next call when this one missed on a database whose fingerprint the previous call had too.
//   4. Part B of the cached chain, always.
// No host synchronisation, no memset: the state block is only ever written by these kernels.
int forward_reusing(const float* packed, const float* desc2d_query, const float* desc3d_db, const float* desc2d_db, int num_leaf, int flags,
                    float scale_factor, float match_threshold, const MatchOut& out, Workspace& w, hipStream_t s) {
    const ColLayout& L = w.L;
    ReuseState* st = w.R.state;
    const size_t words3 = (size_t)L.b * D * L.n2;
    // what every launch of the comparison takes; then per riding launch its share of each piece, its rider count, and the owner role
    DbRider all = {};
    all.P = db_pieces(packed, desc3d_db, desc2d_db, w, num_leaf);
    all.st = st;
    all.stamp = {REUSE_MAGIC, L.b, L.n1p, L.n2, num_leaf, flags};
    all.d3 = reinterpret_cast<const unsigned*>(desc3d_db);
    all.d2db = reinterpret_cast<const unsigned*>(desc2d_db);
    all.n3 = words3;
    all.n2 = words3 * num_leaf;
    DbRider r[DB_RIDER_LAUNCHES];
    for (int k = 0; k < DB_RIDER_LAUNCHES; ++k) {
        r[k] = all;
        r[k].owner = k == 0;
        r[k].blocks = DB_RIDER_BLOCKS[k];
        for (int p = 0; p < DB_PIECES; ++p) db_rider_share(all.P.n[p], k, &r[k].lo[p], &r[k].hi[p]);
    }
    // every window in the whole frame's kernel forms
    w.form_tiles = active_tiles(L);
    const bool rides = db_rider_rides(windowed(w, 0));
    w.rider = rides ? r : nullptr;
    enqueue_cached_query(packed, desc2d_query, w, s);
    w.rider = nullptr;
    if (!rides) launch_db_verify(all, s);
    Workspace wp = w;
    wp.L.gate = &st->miss;
    enqueue_prepare(packed, desc3d_db, desc2d_db, num_leaf, flags, wp, w.R.cache, false, st, s);
    launch_db_snapshot(all.P, st, s);
    // (the leaf-logit table stays out of this path: DbCache::LL is carved and never written here)
    enqueue_cached_rest(packed, desc2d_db, w.R.cache, false, num_leaf, flags, scale_factor, match_threshold, out, w, s);
    return check_launch(1, "forward");
}

int forward_impl(const float* packed, const float* desc2d_query, const float* desc3d_db, const float* desc2d_db, int b,
                 int n1, int n2, int num_leaf, int flags, float scale_factor, float match_threshold, const MatchOut& out,
                 void* ws, size_t ws_bytes, void* stream, ProfileHook* hk) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w, flags)) return e;
    if (!packed || !desc2d_query || !desc3d_db || !desc2d_db) return fail(1, "null input pointer");
    if (int e = check_out(out)) return e;
    if (int e = check_scale(scale_factor)) return e;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // gatsspg_forward_profiled (hk) always takes the plain chain: its launch #0 of a kernel is the whole-frame launch bench.py prices.
    // (The comparison reads 16-byte words: tensors that break the header's alignment rule are simply not compared.)
    const bool aligned = !((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(desc3d_db) | reinterpret_cast<uintptr_t>(desc2d_db)) & 15);
    if (!hk && w.R.present && aligned && !(flags & GATSSPG_FLAG_NO_DB_REUSE))
        return forward_reusing(packed, desc2d_query, desc3d_db, desc2d_db, num_leaf, flags, scale_factor, match_threshold, out, w, s);
    // the state load is fused into the first GATs launch where that kernel supports it (num_leaf == 8, no linear transform)
    const bool fused_load = gats_fuses_state_load(num_leaf, flags, w);
    if (!fused_load) launch_load_state(desc2d_query, desc3d_db, w, s, hk);
    enqueue_rounds(packed, 0, desc2d_db, num_leaf, flags, w, s, hk, fused_load ? desc3d_db : nullptr,
                   fused_load ? desc2d_query : nullptr, nullptr, 0);
    enqueue_tail(packed, w, scale_factor, match_threshold, out, s, hk);
    return check_launch(1, "forward");
}
}  // namespace

extern "C" {

int gatsspg_version(void) { return 413; }   // 413: the workspace of a shape of the reusing plain forward ends in a reuse area (state carried between calls of gatsspg_forward), GATSSPG_FLAG_NO_DB_REUSE; earlier offsets as 412; 412: gatsspg_forward_frames added, nothing else changed (layouts as 411); 411: same layouts as 410; the bound data in the KV partials / database cache changed meaning (slots 0..3: per-wave largest key sum of the tile, summed by kv_final; 4..7: max |V|): a cache written by a 410 library must be re-prepared; 410: message-operator scale of the fp16 modes from a data bound (KV partials carry operand maxima: packed-weights, workspace and database-cache layouts changed); 400: split-16-bit GEMMs on the LDS-DMA loop, power-of-two operand scales of the fp16 modes (packed-weights and workspace layouts changed)
const char* gatsspg_last_error(void) { return g_err; }

size_t gatsspg_packed_weights_bytes(void) { return PACKED_BYTES; }

size_t gatsspg_workspace_bytes(int b, int n1, int n2, int num_leaf) {
    if (check_dims(b, n1, n2, num_leaf)) return 0;
    return carve_workspace(nullptr, b, n1, n2, num_leaf).bytes;
}

int gatsspg_pack_weights(const gatsspg_raw_weights* raw, float* packed, void* stream) {
    if (!raw || !packed) return fail(1, "null argument");
    const void* const* p = reinterpret_cast<const void* const*>(raw);
    for (size_t i = 0; i < sizeof(gatsspg_raw_weights) / sizeof(void*); ++i)
        if (!p[i]) return fail(1, "raw weight pointer #%zu is null", i);
    if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(1, "packed-weights buffer must be 16-byte aligned");
    launch_pack_weights(raw, packed, static_cast<hipStream_t>(stream));
    launch_split_weights(packed, reinterpret_cast<unsigned short*>(packed + PW_TOTAL), static_cast<hipStream_t>(stream));
    return check_launch(1, "pack_weights");
}

int gatsspg_load_state(const float* dq, const float* d3, int b, int n1, int n2, int num_leaf, void* ws, size_t ws_bytes,
                       void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w)) return e;
    if (!dq || !d3) return fail(1, "null descriptor pointer");
    launch_load_state(dq, d3, w, static_cast<hipStream_t>(stream));
    return check_launch(1, "load_state");
}

int gatsspg_store_state(int which, float* out2d, float* out3d, int b, int n1, int n2, int num_leaf, void* ws,
                        size_t ws_bytes, void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w)) return e;
    if (!out2d || !out3d) return fail(1, "null output pointer");
    if (which != 0 && which != 1) return fail(1, "which must be 0 (state) or 1 (normalised final descriptors)");
    launch_store_state(which == 0 ? w.Z : w.MD, out2d, out3d, w, static_cast<hipStream_t>(stream));
    return check_launch(1, "store_state");
}

int gatsspg_gats_layer(const float* packed, int layer, const float* desc2d_db, int b, int n1, int n2, int num_leaf,
                       int flags, void* ws, size_t ws_bytes, void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w, flags)) return e;
    if (!packed || !desc2d_db) return fail(1, "null argument");
    if (layer < 0 || layer >= GATSSPG_NUM_GATS_LAYERS) return fail(1, "GATs layer index %d out of range", layer);
    enqueue_gats(packed, layer, desc2d_db, num_leaf, flags, w, static_cast<hipStream_t>(stream));
    return check_launch(1, "gats_layer");
}

int gatsspg_attn_layer(const float* packed, int layer, int kind, int b, int n1, int n2, int num_leaf, int flags, void* ws,
                       size_t ws_bytes, void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w, flags)) return e;
    if (!packed) return fail(1, "null argument");
    if (layer < 0 || layer >= GATSSPG_NUM_ATTN_LAYERS) return fail(1, "attention layer index %d out of range", layer);
    if (kind != GATSSPG_LAYER_SELF && kind != GATSSPG_LAYER_CROSS) return fail(1, "kind must be SELF or CROSS");
    enqueue_attn(packed, layer, kind, w, static_cast<hipStream_t>(stream));
    return check_launch(1, "attn_layer");
}

int gatsspg_final_proj_norm(const float* packed, int b, int n1, int n2, int num_leaf, void* ws, size_t ws_bytes,
                            void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w)) return e;
    if (!packed) return fail(1, "null argument");
    launch_final_proj_norm(packed + PW_FINAL_W, packed + PW_FINAL_B, w, static_cast<hipStream_t>(stream));
    return check_launch(1, "final_proj_norm");
}

int gatsspg_score_dual_softmax_match(int b, int n1, int n2, int num_leaf, float scale_factor, float match_threshold,
                                     float* conf, int64_t* matches0, int64_t* matches1, float* mscores0,
                                     float* mscores1, void* ws, size_t ws_bytes, void* stream) {
    Workspace w;
    const MatchOut out = {conf, matches0, matches1, mscores0, mscores1};
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w)) return e;
    if (int e = check_out(out)) return e;
    if (int e = check_scale(scale_factor)) return e;
    enqueue_tail(nullptr, w, scale_factor, match_threshold, out, static_cast<hipStream_t>(stream), nullptr);
    return check_launch(1, "score_dual_softmax_match");
}

int gatsspg_forward(const float* packed, const float* desc2d_query, const float* desc3d_db, const float* desc2d_db, int b,
                    int n1, int n2, int num_leaf, int flags, float scale_factor, float match_threshold, float* conf,
                    int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, void* ws, size_t ws_bytes,
                    void* stream) {
    return forward_impl(packed, desc2d_query, desc3d_db, desc2d_db, b, n1, n2, num_leaf, flags, scale_factor,
                        match_threshold, {conf, matches0, matches1, mscores0, mscores1}, ws, ws_bytes, stream, nullptr);
}

int gatsspg_forward_profiled(const float* packed, const float* desc2d_query, const float* desc3d_db,
                             const float* desc2d_db, int b, int n1, int n2, int num_leaf, int flags, float scale_factor,
                             float match_threshold, float* conf, int64_t* matches0, int64_t* matches1, float* mscores0,
                             float* mscores1, void* ws, size_t ws_bytes, void* stream, int kernel_id, int occurrence,
                             void* ev_start, void* ev_stop) {
    if (kernel_id < 0 || kernel_id >= KID_COUNT) return fail(1, "kernel_id %d out of range", kernel_id);
    if (!ev_start || !ev_stop) return fail(1, "null event");
    ProfileHook hk = {kernel_id, occurrence, static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop), {}};
    if (int e = forward_impl(packed, desc2d_query, desc3d_db, desc2d_db, b, n1, n2, num_leaf, flags, scale_factor,
                             match_threshold, {conf, matches0, matches1, mscores0, mscores1}, ws, ws_bytes, stream, &hk))
        return e;
    if (hk.seen[kernel_id] <= occurrence) return fail(1, "kernel %d was launched %d times, occurrence %d never ran", kernel_id, hk.seen[kernel_id], occurrence);
    return 0;
}

#ifdef GATSSPG_PROFILING_BUILD
/* profiling builds only (not part of the public header): per-workgroup timeline of mlp0_kernel */
void gatsspg_debug_set_trace(void* buf) { g_trace = static_cast<unsigned long long*>(buf); }
#endif

size_t gatsspg_db_cache_bytes(int b, int n2) {
    if (b < 1 || n2 < 2) return 0;
    return carve_cache(nullptr, b, n2).bytes;
}

int gatsspg_prepare_database(const float* packed, const float* desc3d_db, const float* desc2d_db, int b, int n2,
                             int num_leaf, int flags, void* cache, size_t cache_bytes, void* ws, size_t ws_bytes,
                             void* stream) {
    Workspace w;
    if (int e = check_ws(ws, ws_bytes, b, 2, n2, num_leaf, w, flags)) return e;   // 2 dummy (zero) query columns
    if (!packed || !desc3d_db || !desc2d_db || !cache) return fail(1, "null argument");
    if (reinterpret_cast<uintptr_t>(cache) & 15) return fail(1, "database cache must be 16-byte aligned");
    const DbCache c = carve_cache(cache, b, n2);
    if (cache_bytes < c.bytes) return fail(1, "database cache too small: %zu < %zu bytes", cache_bytes, c.bytes);
    enqueue_prepare(packed, desc3d_db, desc2d_db, num_leaf, flags, w, c, gats_caches_leaf_logits(num_leaf, flags), nullptr, static_cast<hipStream_t>(stream));
    return check_launch(1, "prepare_database");
}

int gatsspg_forward_cached(const float* packed, const float* desc2d_query, const float* desc2d_db, const void* cache,
                           size_t cache_bytes, int b, int n1, int n2, int num_leaf, int flags, float scale_factor,
                           float match_threshold, float* conf, int64_t* matches0, int64_t* matches1, float* mscores0,
                           float* mscores1, void* ws, size_t ws_bytes, void* stream) {
    Workspace w;
    const MatchOut out = {conf, matches0, matches1, mscores0, mscores1};
    if (int e = check_ws(ws, ws_bytes, b, n1, n2, num_leaf, w, flags)) return e;
    if (!packed || !desc2d_query || !desc2d_db || !cache) return fail(1, "null input pointer");
    if (int e = check_out(out)) return e;
    if (int e = check_scale(scale_factor)) return e;
    const DbCache c = carve_cache(const_cast<void*>(cache), b, n2);
    if (cache_bytes < c.bytes) return fail(1, "database cache too small: %zu < %zu bytes", cache_bytes, c.bytes);
    enqueue_cached(packed, desc2d_query, desc2d_db, c, gats_caches_leaf_logits(num_leaf, flags), num_leaf, flags, scale_factor, match_threshold, out, w,
                   static_cast<hipStream_t>(stream));
    return check_launch(1, "forward_cached");
}

// The cached chain of gatsspg_forward_cached on a frames layout (gatsspg_common.h): the workspace and the outputs are carved for the capacity
// cap1, every kernel takes the frames' own counts by value in its arguments, the cache of ONE database serves every frame with stride 0.
int gatsspg_forward_frames(const float* packed, const float* desc2d_query, const int32_t* n1, const float* desc2d_db, const void* cache,
                           size_t cache_bytes, int b, int cap1, int n2, int num_leaf, int flags, float scale_factor,
                           float match_threshold, float* conf, int64_t* matches0, int64_t* matches1, float* mscores0,
                           float* mscores1, void* ws, size_t ws_bytes, void* stream) {
    Workspace w;
    const MatchOut out = {conf, matches0, matches1, mscores0, mscores1};
    if (b < 1 || b > MAX_FRAMES) return fail(1, "forward_frames takes 1 to %d frames (got %d)", MAX_FRAMES, b);
    if (!n1) return fail(1, "null pointer to the query counts");
    if (int e = check_ws(ws, ws_bytes, b, cap1, n2, num_leaf, w, flags)) return e;
    for (int f = 0; f < b; ++f)
        if (n1[f] < 2 || n1[f] > cap1) return fail(1, "query count of frame %d must be in [2, cap1 = %d] (got %d)", f, cap1, n1[f]);
    if (!packed || !desc2d_query || !desc2d_db || !cache) return fail(1, "null input pointer");
    if (int e = check_out(out)) return e;
    if (int e = check_scale(scale_factor)) return e;
    const DbCache c = carve_cache(const_cast<void*>(cache), 1, n2);
    if (cache_bytes < c.bytes) return fail(1, "database cache too small: %zu < %zu bytes (the cache of ONE database, b = 1)", cache_bytes, c.bytes);
    w.frames = true;
    w.shared_leaf = true;
    for (int f = 0; f < MAX_FRAMES; ++f) w.fcnt[f] = f < b ? n1[f] : 0;
    enqueue_cached(packed, desc2d_query, desc2d_db, c, gats_caches_leaf_logits(num_leaf, flags), num_leaf, flags, scale_factor, match_threshold, out, w,
                   static_cast<hipStream_t>(stream));
    return check_launch(1, "forward_frames");
}

// One GATs layer of a frame batch on the state of a (b, cap1, n2) workspace: the b frames' 3D sides against ONE database's leaves.
int gatsspg_gats_layer_frames(const float* packed, int layer, const float* desc2d_db, const float* leaf_logits, int b, int cap1, int n2,
                              int num_leaf, int flags, int shared_leaf, void* ws, size_t ws_bytes, void* stream) {
    Workspace w;
    if (b < 1 || b > MAX_FRAMES) return fail(1, "gats_layer_frames takes 1 to %d frames (got %d)", MAX_FRAMES, b);
    if (int e = check_ws(ws, ws_bytes, b, cap1, n2, num_leaf, w, flags)) return e;
    if (!packed || !desc2d_db) return fail(1, "null argument");
    if (layer < 0 || layer >= GATSSPG_NUM_GATS_LAYERS) return fail(1, "GATs layer index %d out of range", layer);
    if (shared_leaf && !gats_caches_leaf_logits(num_leaf, flags)) return fail(1, "the shared-leaf form serves num_leaf == 8 without the linear transform");
    if (leaf_logits && !gats_caches_leaf_logits(num_leaf, flags)) return fail(1, "leaf logits exist for num_leaf == 8 without the linear transform only");
    w.frames = true;
    w.shared_leaf = shared_leaf != 0;
    for (int f = 0; f < MAX_FRAMES; ++f) w.fcnt[f] = f < b ? cap1 : 0;   // (a GATs layer touches the 3D side only: the counts do not enter)
    enqueue_gats(packed, layer, desc2d_db, num_leaf, flags, w, static_cast<hipStream_t>(stream), nullptr, nullptr, nullptr, leaf_logits);
    return check_launch(1, "gats_layer_frames");
}

size_t gatsspg_kenc_scratch_bytes(int b, int n) { return (b < 1 || n < 1) ? 0 : kenc_scratch_bytes(b, n); }

int gatsspg_keypoint_encoder(const gatsspg_kenc_weights* kw, const float* kpts, const float* scores, int b, int n,
                             float* out, void* scratch, size_t scratch_bytes, void* stream) {
    if (!kw || !kpts || !scores || !out || !scratch) return fail(1, "null argument");
    if (b < 1 || n < 2) return fail(1, "keypoint encoder needs b >= 1 and n >= 2 (InstanceNorm1d)");
    if (kw->inp_dim != 3 && kw->inp_dim != 4) return fail(1, "inp_dim must be 3 or 4");
    for (int i = 0; i < 4; ++i)
        if (!kw->w[i] || !kw->b[i]) return fail(1, "null encoder weight");
    if (scratch_bytes < kenc_scratch_bytes(b, n)) return fail(1, "scratch too small");
    launch_kenc(kw->w, kw->b, kw->inp_dim, kpts, scores, b, n, out, scratch, static_cast<hipStream_t>(stream));
    return check_launch(1, "keypoint_encoder");
}

}  // extern "C"
