/*
 * gatsspg.h -- C ABI of libgatsspg_hip.so: the MI355X (gfx950) implementation of the OnePose
 * GATsSPG 2D-3D matcher forward pass.
 *
 * The reference has no native/FFI boundary for this path: its boundary is the Python
 * nn.Module `GATsSuperGlue` (reference src/models/GATsSPG_architectures/GATs_SuperGlue.py:143-241,
 * called from inference.py:146 through src/models/GATsSPG_lightning_model.py:36-37).  The entry
 * points below are what a ctypes binding of that module binds; each one
 * names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP), fp32 unless stated, 16-byte aligned, contiguous;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing here
 *     allocates, synchronises, or keeps global mutable state (graph-capture safe);
 *   - return value 0 = OK, non-zero = error; gatsspg_last_error() returns a thread-local
 *     message for the last failing call of the calling thread;
 *   - the only supported descriptor dimension is 256 with 4 heads (hard-coded in the reference
 *     at GATs_SuperGlue.py:35-36,43).
 *
 * Tensor shapes use the reference's names: b batch, n1 = N_2D query keypoints, n2 = N_3D points,
 * num_leaf = per-view 2D descriptors ("leaves") per 3D point.
 */
#ifndef GATSSPG_H
#define GATSSPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GATSSPG_D 256
#define GATSSPG_HEADS 4
#define GATSSPG_NUM_ATTN_LAYERS 8 /* 'self','cross' x4  (GATs_SuperGlue.py:162) */
#define GATSSPG_NUM_GATS_LAYERS 4 /* 'GATs' x4 */

/* GraphAttentionLayer flags (GATs.py:14-16, hparams include_self/additional/with_linear_transform) */
#define GATSSPG_FLAG_INCLUDE_SELF 1
#define GATSSPG_FLAG_ADDITIONAL 2
#define GATSSPG_FLAG_WITH_LINEAR_TRANSFORM 4
/* Arithmetic of the three big GEMMs of every attention layer (QKV projection, merge+mlp.0, mlp.3), selected PER CALL --
 * the library never reads the environment:
 *   bit clear (default): exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the reference's arithmetic (GATs_SuperGlue.py:191-193);
 *   GATSSPG_FLAG_PREC_BF16X3: split-bf16 -- every fp32 operand is a sum of two bf16 terms and each product three
 *     v_mfma_f32_32x32x16_bf16 with fp32 accumulation (BASELINE configs[2] "bf16 MFMA").  Measured against the reference
 *     (tests/test_hip_parity.py runs every golden case under both modes): conf within 1e-6 abs of the fp32 forward; raw
 *     arg-max indices identical except where the reference's own top-2 entries are closer than 1e-3 relative (1-2 of
 *     64000 on the random-weight b=8 fixture, none on the others); thresholded matches identical on every fixture.
 *   GATSSPG_FLAG_PREC_BF16X6: six-term split-bf16 -- every fp32 operand is the EXACT sum of three bf16 terms (3 x 8 = 24
 *     mantissa bits) and each product the six largest of the nine term products; what is dropped is <= 2^-24 |ab|, one
 *     fp32 rounding of the product, and the accumulation is the MFMA's fp32 accumulation -- fp32-class arithmetic on the
 *     bf16 matrix pipe (the tests hold it to the fp32 mode's own tie-gap tolerance).  The two precision bits are exclusive.
 * final_proj, GATs, the KV pass of the linear attention and all reductions are fp32 in every mode; the score contraction of the dual
 * softmax is fp32 in the three-term modes (BF16X3, FP16X3) and runs on the same split arithmetic as the GEMMs in the fp32-class
 * modes (BF16X6, FP16X4: score_exp_sp_kernel, exact products of the split unit-norm descriptors). */
#define GATSSPG_FLAG_PREC_BF16X3 0x100
#define GATSSPG_FLAG_PREC_BF16X6 0x200
/*   GATSSPG_FLAG_PREC_FP16X3 / _FP16X4: two-term split on IEEE fp16 -- every fp32 operand is x1 + x2 with x1 = RNE_fp16(x),
 *     x2 = RNE_fp16(x - x1), i.e. 2 x 11 significand bits with a signed remainder (|x - x1 - x2| <= 2^-23 |x|; bf16x3: 2^-16), both
 *     conversions saturating at +-65504 (MODE.FP16_OVFL) so that an out-of-range operand never becomes infinity.  Every operand is
 *     multiplied by an EXACT power of two before the split and the accumulators are scaled back (ABI 400), so that the second term
 *     stays a normal fp16 number for small operands: weights per matrix at pack time (largest entry to [2^13, 2^14): the 2^-23
 *     bound holds down to |w| ~ 2^-24 max|W|), activations by 2^4 (bound holds down to |x| ~ 2^-7, absolute error 2^-29 below;
 *     exact two-term range +-8188, saturating beyond), the message operator M_h of every (segment, head) by a power of two taken from a
 *     RIGOROUS bound of its entries, |M_h| <= (largest row-L1 norm of head h's merge-folded mlp.0 half) * max |V_h| * KS_h, KS_h >= the
 *     largest key sum max_d sum_m K_h[d][m] (taken as a sum over the 64-column tiles of their largest key sums: one outlier key does not
 *     move it), both data terms carried by the KV partials (layout of ABI 410; round 5 used n_source * max K_h * max |V_h| there, and the
 *     ABI-400 form, 2^-(ceil(log2 n_source) + 6) of the weight scale, never looked at the data and could saturate silently).
 *     FP16X3: the three leading products on v_mfma_f32_32x32x16_f16 -- the matrix-pipe time of bf16x3 (BASELINE configs[3] names
 *     fp16; a SINGLE fp16 term fails the parity bar like a single bf16 term does).  FP16X4: all four products, the exact product
 *     of the split operands with fp32 accumulation -- fp32-class results in four MFMAs where bf16x6 needs six.  Measured parity in
 *     DESIGN.md 12d / tests/test_hip_parity.py (test_split_modes_are_scale_invariant: weights of 1e-3 .. 5e-5, activations of 0.003 .. 1).
 *     The four precision bits are exclusive. */
#define GATSSPG_FLAG_PREC_FP16X3 0x400
#define GATSSPG_FLAG_PREC_FP16X4 0x800
/* gatsspg_forward only: always enqueue the plain chain, never look at or write the workspace's reuse area (see gatsspg_forward).  Not set by
 * default.  Same results, bit for bit; a caller whose database changes on every call saves the comparison pass with it. */
#define GATSSPG_FLAG_NO_DB_REUSE 0x1000 /* not a GraphAttentionLayer or arithmetic flag: which chain gatsspg_forward enqueues */
/* layer kinds for gatsspg_attn_layer (GATs_SuperGlue.py:55-64) */
#define GATSSPG_LAYER_SELF 0
#define GATSSPG_LAYER_CROSS 1

/* Raw parameter pointers, exactly the tensors of the reference state_dict that forward() uses
 * (SURVEY.md 8(b)); index [i] runs over the 4 GATs layers (gnn.layers.{0,3,6,9}) or the 8
 * AttentionPropagation layers (gnn.layers.{1,2,4,5,7,8,10,11}). */
typedef struct gatsspg_raw_weights {
    const float* gats_W[GATSSPG_NUM_GATS_LAYERS];       /* [256,256]  h @ W           (GATs.py:25,40) */
    const float* gats_a[GATSSPG_NUM_GATS_LAYERS];       /* [512,1]                    (GATs.py:27)    */
    const float* proj_w[GATSSPG_NUM_ATTN_LAYERS][3];    /* attn.proj.{0,1,2}.weight [256,256,1] (:91)  */
    const float* proj_b[GATSSPG_NUM_ATTN_LAYERS][3];    /* attn.proj.{0,1,2}.bias   [256]              */
    const float* merge_w[GATSSPG_NUM_ATTN_LAYERS];      /* attn.merge.weight [256,256,1]        (:90)  */
    const float* merge_b[GATSSPG_NUM_ATTN_LAYERS];      /* attn.merge.bias   [256]                     */
    const float* mlp0_w[GATSSPG_NUM_ATTN_LAYERS];       /* mlp.0.weight [512,512,1]             (:108) */
    const float* mlp0_b[GATSSPG_NUM_ATTN_LAYERS];       /* mlp.0.bias   [512]                          */
    const float* mlp3_w[GATSSPG_NUM_ATTN_LAYERS];       /* mlp.3.weight [256,512,1]                    */
    const float* mlp3_b[GATSSPG_NUM_ATTN_LAYERS];       /* mlp.3.bias   [256]                          */
    const float* final_w;                               /* final_proj.weight [256,256,1]        (:170) */
    const float* final_b;                               /* final_proj.bias   [256]                     */
} gatsspg_raw_weights;

/* KeypointEncoder parameters (GATs_SuperGlue.py:131-140; built, never called by forward). */
typedef struct gatsspg_kenc_weights {
    const float* w[4]; /* encoder.{0,3,6,9}.weight [c_out, c_in, 1], c = inp,32,64,128,256 */
    const float* b[4]; /* encoder.{0,3,6,9}.bias */
    int inp_dim;       /* 3 (kenc_2d) or 4 (kenc_3d) */
} gatsspg_kenc_weights;

int gatsspg_version(void);
const char* gatsspg_last_error(void);

/* Size in bytes of the packed-weights blob / of the workspace for a given problem. */
size_t gatsspg_packed_weights_bytes(void);
size_t gatsspg_workspace_bytes(int b, int n1, int n2, int num_leaf);

/* One-time weight preparation (replaces nothing in the reference; it is what
 * load_state_dict + .cuda() is to it).  Re-orders the q/k/v projection rows head-major, folds
 * merge into mlp.0 (W0[:,256:] @ Wm), folds W @ a[:256], W @ a[256:] of each GATs layer, and appends the bf16 hi/lo
 * planes of the three big operators of every attention layer (used by GATSSPG_FLAG_PREC_BF16X3 / _BF16X6 calls). */
int gatsspg_pack_weights(const gatsspg_raw_weights* raw, float* packed, void* stream);

/* Whole forward: GATsSuperGlue.forward, GATs_SuperGlue.py:179-241, for all b samples.
 *   desc2d_query [b,256,n1]  desc3d_db [b,256,n2]  desc2d_db [b,256,n2*num_leaf]
 *   conf [b,n1,n2]; matches0 [b,n1] int64; matches1 [b,n2] int64; mscores0 [b,n1]; mscores1 [b,n2]
 * n1 >= 2 and n2 >= 2 (the reference raises for a single point, and returns early for 0). */
/* DATABASE REUSE.  The 3D database is one per object and a caller of the reference's forward(data) passes the same tensors for every frame of
 * a sequence, so on shapes of more than 64 column tiles -- b * (round_up(n1, 128) + round_up(n2, 128)) / 64 > 64; smaller frames are bound by
 * launches and run the plain chain -- gatsspg_forward keeps, in a reuse area at the END of the workspace, what the first three GNN layers
 * derive from the database and the weights alone (the cache of the amortised mode below), together with a bitwise snapshot of desc3d_db,
 * desc2d_db and the packed-weight ranges that work depends on (GATs layer 0, attention layers 0 and 1).  Every call compares the
 * caller's tensors with the snapshot, ALL of them, word for word, on the device (168 MB of reads at 1000 x 7000 x 8 leaves, under the call's
 * first launches, which work on the query alone: about 5 us of the 28 us the pass takes alone, fp32; a launch of its own otherwise); if
 * they are equal it skips that work (about 12 % of the frame's matrix flops and one pass over the leaves), otherwise it redoes it from this
 * call's inputs.  There is no host synchronisation and the launch sequence is the same either way (graph-capture safe): the kernels of the
 * skipped part are launched and return at once.  A snapshot is taken (a copy of the database) when a call misses on a database whose
 * fingerprint -- a sum over 8 KB of it -- the previous call had too: a constant database misses twice and hits from the third call on, a
 * database that changes on every call never pays the copy.  The fingerprint never decides a hit.
 *   - Results are BIT FOR BIT those of the plain chain (GATSSPG_FLAG_NO_DB_REUSE): the windowed launches take the whole frame's kernel forms.
 *   - The workspace therefore carries state between calls of gatsspg_forward.  One workspace serves one stream at a time, as before.
 *     Overwriting it is harmless and costs the next two calls a miss: a hit reads nothing of the area that the comparison has not covered
 *     -- the snapshot against the caller's tensors, the cache against a second copy of itself, the stamp of the state block (magic value,
 *     b, round_up(n1, 128), n2, num_leaf, flags) -- so the same memory may serve calls of other shapes, flags or entry points in between.
 *     Changing the database or the weights in place is detected (it is a mismatch like any other).
 *   - The price where it never pays.  A call that misses redoes the database-side work on a 3D-side window and the rest on a query-side
 *     window, each launch about as long as the whole frame's, on top of the comparison pass.  Measured at 1000 x 7000 x 8 leaves, fp32, with
 *     two databases alternated call by call (never a hit, never a snapshot): 1065 against 1140 frames/s with 4 frames in flight (-7 %),
 *     1.134 against 1.014 ms one frame at a time (+12 %).  A caller whose database changes on every call sets GATSSPG_FLAG_NO_DB_REUSE and
 *     is where it was; a caller with one database per sequence pays two such calls per sequence.
 * gatsspg_forward_profiled always runs the plain chain.
 * The area's state block is the LAST 256 bytes of a workspace of such a shape, at gatsspg_workspace_bytes(b, n1, n2, num_leaf) - 256:
 * sixteen int32 words, for a caller (or a test) that wants to know what the last call did, read after synchronising the stream: [0..5] the
 * stamp (a magic value, b, round_up(n1, 128), n2, num_leaf, flags), [6] the fingerprint of the last call's database, [7] snapshot_valid,
 * [8] miss (during a call: a difference was found; 0 again afterwards), [9] strike (its fingerprint was the previous call's), [10] hit (1: the
 * last call reused the cache; 0: it redid the work).  A workspace of a smaller shape has no area and ends as it did before ABI 413. */
int gatsspg_forward(const float* packed, const float* desc2d_query, const float* desc3d_db,
                    const float* desc2d_db, int b, int n1, int n2, int num_leaf, int flags,
                    float scale_factor, float match_threshold, float* conf, int64_t* matches0,
                    int64_t* matches1, float* mscores0, float* mscores1, void* ws, size_t ws_bytes,
                    void* stream);

/* Same forward, with a HIP-event bracket (hipEvent_t, created by the caller, recorded on `stream`)
 * around the `occurrence`-th launch of one kernel -- how bench.py times the dominant kernel live.
 * kernel_id: 0 load_state (only when the first GATs launch cannot fuse it), 1 gats, 2 qkv_kv, 3 kv_final (KV sums + the message operators M_t of mlp.0), 4 retired (the former attn_apply launch: folded into 3 and 5),
 * 5 mlp0, 6 stat_final, 7 mlp3, 8 final_proj_norm, 9 score_exp, 10 conf_finalize, 11 match_tail, 12 gats_wlt,
 * 13 softmax_stats (max-subtracting path only). */
int gatsspg_forward_profiled(const float* packed, const float* desc2d_query, const float* desc3d_db,
                             const float* desc2d_db, int b, int n1, int n2, int num_leaf, int flags,
                             float scale_factor, float match_threshold, float* conf, int64_t* matches0,
                             int64_t* matches1, float* mscores0, float* mscores1, void* ws, size_t ws_bytes,
                             void* stream, int kernel_id, int occurrence, void* ev_start, void* ev_stop);

/* ---- amortised mode: per-object database cache ------------------------------------
 * The 3D database (desc3d_db + its leaves desc2d_db) is constant per object (inference.py:113-130) while the
 * reference recomputes -- and re-uploads, inference.py:86-90 -- everything per frame.  gnn.layers.0 (GATs),
 * the 3D side of gnn.layers.1 (self), the 3D-side projections / KV sums of gnn.layers.2 (cross) and the leaf logits
 * of the later GATs layers (num_leaf == 8, no linear transform) do not depend on the query frame; gatsspg_prepare_database computes them once, gatsspg_forward_cached skips them.
 * Those stages run on ONE-SIDE WINDOWS of the frame (the 3D columns when the cache is prepared, the query columns in the cached forward), and a
 * stage with two kernel forms picks its form by the 64-column tiles of its own launch: b * round_up(n, 128) / 64 for a window,
 * b * (round_up(n1, 128) + round_up(n2, 128)) / 64 for the plain forward.  Results are bit-identical to gatsspg_forward (same kernels, same
 * fixed-order reductions) when every windowed launch takes the form the whole-frame launch takes; two thresholds separate forms that associate
 * their sums differently: the fp32 mlp.3 tile (up to 64 tiles: the 64x64 tile that splits K over two wave groups and adds the halves last;
 * above: the tall tile) and the fp16x3 / fp16x4 mlp.0 tile (tiles / 2 in [48, 64]: the 128-column tile; otherwise the 64-column tile, which
 * walks the columns of an InstanceNorm partial from another start).  The other launch-size thresholds (register-diet forms of the fp32 qkv_kv /
 * mlp.0, two- / three-stage ring of the fp16 mlp.3) separate forms that issue the same MFMAs in the same order.  bf16x3 / bf16x6 have one form
 * per stage and are always bit-identical.
 * Otherwise (the fp32 headline shape: 1000 x 7000 is 126 tiles, its query window 16) the two differ by the re-association noise of those sums
 * and give the same matches: measured max |d conf| 3.5e-8 (fp32, 100 x 4000) and 1.1e-8 (fp16x4, 100 x 6000) on conf entries up to 5e-3,
 * asserted below 2e-5 with identical matches0 / matches1 (tests/test_gats_stage_edges.py::test_database_cache_at_form_edges).
 * All of this WHEN THE CACHE WAS PREPARED UNDER THE SAME `flags` AND
 * PACKED WEIGHTS as the call that consumes it.  The library does not record them in the cache (the Python wrapper does, and refuses a
 * mismatch); a C caller that mixes arithmetics gets a well-defined result -- the cached stages in the arithmetic of the prepare call, the
 * rest in the arithmetic of the forward call -- within the two arithmetics' difference of the plain forward: since round 6 the KV sums of
 * EVERY arithmetic carry the operand maxima that the fp16 modes' message-operator scale reads (ABI 410), never uninitialised slots
 * (tests/test_hip_parity.py::test_database_cache_prepared_under_other_flags_is_valid_input_for_the_fp16_modes).  A cache prepared with OTHER
 * WEIGHTS is simply wrong.  The cache does not depend on n1.
 * ws for prepare: at least gatsspg_workspace_bytes(b, 2, n2, num_leaf). */
size_t gatsspg_db_cache_bytes(int b, int n2);
int gatsspg_prepare_database(const float* packed, const float* desc3d_db, const float* desc2d_db, int b, int n2,
                             int num_leaf, int flags, void* cache, size_t cache_bytes, void* ws, size_t ws_bytes,
                             void* stream);
int gatsspg_forward_cached(const float* packed, const float* desc2d_query, const float* desc2d_db, const void* cache,
                           size_t cache_bytes, int b, int n1, int n2, int num_leaf, int flags, float scale_factor,
                           float match_threshold, float* conf, int64_t* matches0, int64_t* matches1,
                           float* mscores0, float* mscores1, void* ws, size_t ws_bytes, void* stream);

/* ---- ragged frame batch against ONE database (the serving case: many frames of one object) ----------------
 * b <= GATSSPG_MAX_FRAMES frames in one chain of launches; frame i has its own query count n1[i], 2 <= n1[i] <= cap1, and all
 * frames run against one database and ONE b = 1 cache (gatsspg_prepare_database(b = 1)): nothing of the database is replicated.
 *   desc2d_query [b,256,cap1]: frame i's descriptors in columns [0, n1[i]); the columns behind them are never read
 *   n1: HOST memory, b int32 entries, read when the call is enqueued (the counts travel by value in the kernel arguments: nothing is
 *       allocated, copied or synchronised, and the call can be captured into a graph -- which then holds these counts)
 *   desc2d_db [1,256,n2*num_leaf]; cache / cache_bytes: as for gatsspg_forward_cached with b = 1
 *   conf [b,cap1,n2]; matches0 [b,cap1]; matches1 [b,n2]; mscores0 [b,cap1]; mscores1 [b,n2]
 *   ws: at least gatsspg_workspace_bytes(b, cap1, n2, num_leaf)
 * Frame i's outputs -- conf rows [0, n1[i]), matches0 / mscores0 [0, n1[i]), matches1 / mscores1 -- are BIT FOR BIT what
 * gatsspg_forward_cached(b = 1, n1 = n1[i]) returns for that frame alone, in every arithmetic and flag combination: every loop
 * bound, mask, partial count and partition is the frame's own, and a stage whose kernel form depends on the launch size runs every
 * frame on the form it takes alone.  Past a count: matches0 = -1 and mscores0 = 0; the conf rows [n1[i], cap1) of frame i are NOT
 * WRITTEN (28 KB each at 7000 points): they keep whatever the buffer held.
 * Refused with a message, before any launch: b < 1, b > GATSSPG_MAX_FRAMES, a count below 2 or above cap1, a null pointer, a
 * cache smaller than gatsspg_db_cache_bytes(1, n2). */
#define GATSSPG_MAX_FRAMES 32
int gatsspg_forward_frames(const float* packed, const float* desc2d_query, const int32_t* n1, const float* desc2d_db,
                           const void* cache, size_t cache_bytes, int b, int cap1, int n2, int num_leaf, int flags,
                           float scale_factor, float match_threshold, float* conf, int64_t* matches0, int64_t* matches1,
                           float* mscores0, float* mscores1, void* ws, size_t ws_bytes, void* stream);

/* One GATs layer (layer = 0..3) of a frame batch, on the state of a (b, cap1, n2) workspace: the 3D sides of the b frames against ONE
 * database's leaves desc2d_db [1,256,n2*num_leaf].  leaf_logits: NULL, or that layer's cached logits ([tiles][32] floats; num_leaf == 8
 * without the linear transform).  shared_leaf != 0: the kernel that reads each 4-point leaf tile once for a group of 4 frames (what
 * gatsspg_forward_frames runs; num_leaf == 8 without the linear transform only); 0: the per-frame kernel with the database at frame
 * stride 0.  Both write, frame by frame, bit for bit what gatsspg_gats_layer writes for that frame with its own copy of the leaves. */
int gatsspg_gats_layer_frames(const float* packed, int layer, const float* desc2d_db, const float* leaf_logits, int b, int cap1,
                              int n2, int num_leaf, int flags, int shared_leaf, void* ws, size_t ws_bytes, void* stream);

/* ---- per-stage entry points (the stages gatsspg_forward is made of; used by the parity
 *      tests to check each kernel against the oracle).  They operate on the workspace state. */

/* loads desc2d_query / desc3d_db into the padded channel-major state (GATs_SuperGlue.py:192-193) */
int gatsspg_load_state(const float* desc2d_query, const float* desc3d_db, int b, int n1, int n2,
                       int num_leaf, void* ws, size_t ws_bytes, void* stream);
/* copies the current state (which=0) or the normalised final descriptors (which=1) out of the
 * workspace as [b,256,n1] and [b,256,n2] */
int gatsspg_store_state(int which, float* out2d, float* out3d, int b, int n1, int n2, int num_leaf,
                        void* ws, size_t ws_bytes, void* stream);
/* GraphAttentionLayer.forward (GATs.py:35-88) on the state's 3D side; layer = 0..3 */
int gatsspg_gats_layer(const float* packed, int layer, const float* desc2d_db, int b, int n1, int n2,
                       int num_leaf, int flags, void* ws, size_t ws_bytes, void* stream);
/* one 'self' or 'cross' layer, both sides: AttentionalGNN.forward branch GATs_SuperGlue.py:55-64
 * = 2x AttentionPropagation.forward (:111-113) + residual; layer = 0..7; flags: only the GATSSPG_FLAG_PREC_* bits matter */
int gatsspg_attn_layer(const float* packed, int layer, int kind, int b, int n1, int n2, int num_leaf,
                       int flags, void* ws, size_t ws_bytes, void* stream);
/* final_proj + F.normalize (GATs_SuperGlue.py:209-213) */
int gatsspg_final_proj_norm(const float* packed, int b, int n1, int n2, int num_leaf, void* ws,
                            size_t ws_bytes, void* stream);
/* score einsum / scale, dual softmax, mutual-NN matching (GATs_SuperGlue.py:217-237).  Any scale_factor > 0:
 * 1/scale_factor <= 80 takes the fused one-pass form, smaller values the max-subtracting form of torch.softmax. */
int gatsspg_score_dual_softmax_match(int b, int n1, int n2, int num_leaf, float scale_factor,
                                     float match_threshold, float* conf, int64_t* matches0,
                                     int64_t* matches1, float* mscores0, float* mscores1, void* ws,
                                     size_t ws_bytes, void* stream);

/* KeypointEncoder.forward (GATs_SuperGlue.py:138-140): kpts [b,n,inp_dim-1], scores [b,n]
 * -> out [b,256,n].  scratch: at least gatsspg_kenc_scratch_bytes(b,n) bytes. */
size_t gatsspg_kenc_scratch_bytes(int b, int n);
int gatsspg_keypoint_encoder(const gatsspg_kenc_weights* w, const float* kpts, const float* scores,
                             int b, int n, float* out, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GATSSPG_H */
