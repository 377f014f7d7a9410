// Host-side launcher prototypes shared between the kernel translation units and the C ABI.
#pragma once
#include "gatsspg_common.h"

namespace gatsspg {

// Kernel ids (also the `kernel_id` of gatsspg_forward_profiled, include/gatsspg.h)
enum KernelId {
    KID_LOAD_STATE = 0, KID_GATS = 1, KID_QKV_KV = 2, KID_KV_FINAL = 3, KID_ATTN_APPLY = 4 /* retired: folded into kv_final + mlp0 */, KID_MLP0 = 5,
    KID_STAT_FINAL = 6, KID_MLP3 = 7, KID_FINAL_PROJ = 8, KID_SCORE_EXP = 9, KID_CONF_FINALIZE = 10,
    KID_MATCH_TAIL = 11, KID_GATS_WLT = 12, KID_SOFTMAX_STATS = 13, KID_COUNT = 14
};

// Optional HIP-event bracket around the `occurrence`-th launch of kernel `kernel_id` inside one forward
// (events live on the same stream as the kernels).  nullptr = no instrumentation.
struct ProfileHook {
    int kernel_id, occurrence;
    hipEvent_t start, stop;
    int seen[KID_COUNT];
};
inline bool hook_hit(ProfileHook* h, int kid) { return h && h->kernel_id == kid && h->seen[kid] == h->occurrence; }
inline void hook_before(ProfileHook* h, int kid, hipStream_t s) {
    if (hook_hit(h, kid)) (void)hipEventRecord(h->start, s);
}
inline void hook_after(ProfileHook* h, int kid, hipStream_t s) {
    if (hook_hit(h, kid)) (void)hipEventRecord(h->stop, s);
    if (h) h->seen[kid]++;
}
#define GATSSPG_LAUNCH(hook, kid, stream, ...)      \
    do {                                            \
        hook_before(hook, kid, stream);             \
        hipLaunchKernelGGL(__VA_ARGS__);            \
        hook_after(hook, kid, stream);              \
    } while (0)

// Tuning knobs.  The product library has NO environment lookups: every knob is its compiled-in default.  A library built
// with -DGATSSPG_TUNING (python -m onepose_amd.build_ext --tuning -> libgatsspg_hip_tuning.so, never loaded by the
// package) reads GATSSPG_<NAME> from the environment: only the shape thresholds that choose between two product kernels
// (DIET_MIN_TILES, SMALL_NT3, SP_MLP0_WIDE_MIN / _MAX, SP_NST2).  Compile-time alternatives are A/B-timed as two builds (tools/ab_libs.py).
int tuning_knob(const char* name, int dflt);

// Kernels whose dynamic LDS request exceeds the 64 KiB default need the limit raised once per device.  The once-flag
// lives in a function template instantiated per KERNEL (the kernel is a non-type template argument), so two variants
// that merely share a signature never share it.
template <auto Kernel>
void allow_big_lds() {
    static bool done[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !done[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024 - 2048);
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
}

// gatsspg_gemm_kernels.hip
#ifdef GATSSPG_PROFILING_BUILD
extern unsigned long long* g_trace;  // per-workgroup timeline buffer of mlp0_kernel (nullptr = off)
#endif
void launch_qkv_kv(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);   // a: attn_layer(packed, layer)
// KV / ksum sums of every active SOURCE segment + the message operators M_t of their TARGET segments (cross: the other side of
// the frame) for mlp.0.  kv_src: nullptr, or (amortised mode) the cached final KV sums [b][4][KVP] of the 3D-side sources, used
// instead of the partials.
void launch_kv_final(const AttnLayer& a, const Workspace& w, int cross, const float* kv_src, hipStream_t s, ProfileHook* hk = nullptr);
void launch_mlp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
// gatsspg_split_kernels.hip: the same three GEMMs on the LDS-DMA split-16-bit loop (gemm_split_glds.h), for is_fp16(w.prec)
void launch_qkv_kv_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
void launch_mlp0_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
void launch_mlp3_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
// score contraction + exp on the split loop (fp32-class modes only: bf16x6, fp16x4): A = the 16-bit planes of the query descriptors
// written by final_proj_norm_kernel (w.MDTp), B = the fp32 3D descriptors.  Same outputs and partial layout as launch_score_exp.
bool score_on_split_loop(Arith prec, int shifted);
void launch_score_exp_sp(const Workspace& w, float* conf, float scale, hipStream_t s, ProfileHook* hk = nullptr);
constexpr int SCORE_SPLIT_SCALE_LOG2 = 10;   // unit-norm descriptors (|x| <= 1) are multiplied by 2^10 before the fp16 split
void launch_final_proj_norm(const float* Wf, const float* bf, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
// shifted = 0: E = exp(S) into conf + row/col sum partials (|S| <= 80); 1: raw scores S into conf (max-subtracting path)
void launch_score_exp(const Workspace& w, float* conf, float scale, int shifted, hipStream_t s, ProfileHook* hk = nullptr);
int score_tile_rows();   // rows / columns of a score tile = what one column / row partial sums over (conf_finalize needs the counts)
int score_tile_cols();
void launch_gats_wlt(const GatsLayer& g, const float* P, const Workspace& w, int add_h, hipStream_t s, ProfileHook* hk = nullptr);
void launch_split_weights(float* packed, unsigned short* packedb, hipStream_t s);   // also writes the fp16 plane scales (AttnW::SC) into `packed`

// gatsspg_stream_kernels.hip
void launch_load_state(const float* dq, const float* d3, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
// copies compact [b,256,n] columns of one or both sides into `dst` ([256][ld]); a null side is left untouched
void launch_load_columns(const float* c2, const float* c3, float* dst, const Workspace& w, hipStream_t s);
void launch_store_state(const float* src, float* out2d, float* out3d, const Workspace& w, hipStream_t s, ProfileHook* hk = nullptr);
// the final KV sums of the 3D-side segments (w.kvfin, written by launch_kv_final) into a database cache's kvY [b][4][KVP]
void launch_store_kv_sums(float* kvY, const Workspace& w, hipStream_t s);
// the cached chain's two copies in one launch: compact [b,256,n2] tensors s0 / s1 into the 3D-side columns of d0 / d1 ([256][ld])
void launch_load_db_columns(const float* s0, float* d0, const float* s1, float* d1, const Workspace& w, hipStream_t s);
// The plain forward's database reuse.  The comparison (db_verify_share, gatsspg_common.h): st->miss (left 0 by the previous
// call) becomes 1 unless every 16-byte word of the pieces equals its snapshot, the snapshot is valid and was taken under r.stamp; also
// st->strike (the database's fingerprint, a sum over a strided sample of r.d3 [n3 words] and r.d2db [n2 words], equals the previous call's)
// and the new fingerprint and stamp.  It rides on the fp32 GEMM launches of the query window where db_rider_rides says so (Workspace::rider;
// launch_qkv_kv and launch_mlp then start r[k].blocks more workgroups); launch_db_verify is the same comparison as one launch of its own,
// for every other frame (r: pieces, state, stamp and tensors; shares and roles are set here).
// launch_db_settle, the last launch of the prepare chain (one workgroup, never gated): on a miss launch_store_kv_sums' work; st->hit = !miss,
// st->copy = miss with a strike, st->snapshot_valid set by such a miss and cleared by any other; st->miss cleared for the next call.
// launch_db_snapshot: copies the pieces into the snapshot where st->copy says so.
bool db_rider_rides(const Workspace& wx);   // wx: the query window of the call (gatsspg_gemm_kernels.hip)
void launch_db_settle(float* kvY, const Workspace& w, ReuseState* st, hipStream_t s);
void launch_db_verify(DbRider r, hipStream_t s);
void launch_db_snapshot(const DbPieces& P, ReuseState* st, hipStream_t s);
// h3: where the layer reads the 3D-point descriptors from: nullptr = the state Z; otherwise the caller's compact
// [b,256,n2] tensor (first layer of a forward: the state load is fused, `dq` is copied into the 2D side by spare workgroups)
void launch_gats(const GatsLayer& g, const float* leaves, int num_leaf, int flags, float* dst, const Workspace& w, hipStream_t s,
                 ProfileHook* hk = nullptr, const float* h3 = nullptr, const float* dq = nullptr, const float* cached_logits = nullptr);
// per-object cache of the leaf logits (amortised mode): [nlayers][b][tiles][32] floats, gats_leaf_logit_floats per layer;
// launch_gats(..., cached_logits = that layer's block) then skips the leaf . u1 products
bool gats_caches_leaf_logits(int num_leaf, int flags);
size_t gats_leaf_logit_floats(int b, int n2);
void launch_gats_leaf_logits(const GatsLayer& first, int nlayers, const float* leaves, float* cl, const Workspace& w, hipStream_t s);   // first of nlayers consecutive layers
// true if launch_gats can take h3 / dq for this configuration (fused state load)
bool gats_fuses_state_load(int num_leaf, int flags, const Workspace& w);
struct MatchOut { float* conf; int64_t *matches0, *matches1; float *mscores0, *mscores1; };   // the five outputs of a forward (include/gatsspg.h)
void launch_dual_softmax_match(const Workspace& w, const MatchOut& out, int shifted, float match_threshold, hipStream_t s,
                               ProfileHook* hk = nullptr);
void launch_pack_weights(const void* raw_struct_host, float* packed, hipStream_t s);
size_t kenc_scratch_bytes(int b, int n);
void launch_kenc(const float* const* w, const float* const* bias, int inp_dim, const float* kpts, const float* scores,
                 int b, int n, float* out, void* scratch, hipStream_t s);

}  // namespace gatsspg
