/*
 * C ABI of the MI355X (gfx950) SuperGlue 2D-2D matcher -- OnePose's other matcher, used by the per-frame
 * object detector (local_feature_2D_detector.py) and by offline SfM mapping (sfm/match_features.py).
 *
 * Replaces, on the GPU, the forward of the reference module
 *   src/models/matchers/SuperGlue/superglue.py:207-276  (SuperGlue.forward)
 * with its helpers MLP (:47-59), normalize_keypoints (:62-69), KeypointEncoder (:72-82), attention /
 * MultiHeadedAttention / AttentionalPropagation / AttentionalGNN (:85-133), log_sinkhorn_iterations and
 * log_optimal_transport (:136-170).
 *
 * Conventions (same as gatsspg.h / superpoint.h): every pointer is a DEVICE pointer to contiguous fp32 /
 * int32 / int64 data unless stated otherwise; all work is enqueued on `stream`; the library never allocates
 * and never synchronises; functions return 0 on success or a negative code, with text available from
 * sg_last_error().  Arithmetic is fp32 throughout (v_mfma_f32_32x32x2_f32 and fp32 VALU).
 *
 * Shapes (reference layout): keypoints [b][n][2] (x, y), scores [b][n], descriptors [b][256][n].
 * descriptor_dim is 256, the keypoint encoder is [32, 64, 128, 256], 4 heads of 64 dimensions.
 * n0, n1 >= 1 (the reference returns before any compute when a side is empty, :221-231; so does the module).
 * Layer kinds: a HOST array of n_layers ints, SG_LAYER_SELF or SG_LAYER_CROSS (GNN_layers).
 */
#ifndef ONEPOSE_AMD_SUPERGLUE_H
#define ONEPOSE_AMD_SUPERGLUE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* sg_stream_t; /* hipStream_t */

#define SG_DESC_DIM 256
#define SG_HEADS 4
#define SG_MAX_LAYERS 64
#define SG_LAYER_SELF 0
#define SG_LAYER_CROSS 1
#define SG_MAX_ITEMS 64 /* items of one ragged batch */
/* float tensors of the reference state_dict (num_batches_tracked skipped): bin_score, 26 of kenc,
 * 16 per GNN layer, 2 of final_proj */
#define SG_NUM_RAW(n_layers) (29 + 16 * (n_layers))

int sg_version(void);
const char* sg_last_error(void);

/* Weight packing (reference :180-205, state_dict order).  `raw` is a HOST array of SG_NUM_RAW(n_layers)
 * DEVICE pointers, one per float tensor of the state_dict in its order, num_batches_tracked skipped.
 * Packing permutes the rows of the q / k / v projections (weights and biases) and the columns of `merge`
 * so that head h occupies channels h*64 .. h*64+63 (the reference's view(b, 64, 4, n) puts channel c in
 * head c % 4, dimension c / 4, :101-103); the permutation is exact. */
size_t sg_packed_weights_bytes(int n_layers);
int sg_pack_weights(const float* const* raw, int n_layers, float* packed, sg_stream_t stream);

size_t sg_workspace_bytes(int b, int n0, int n1);

/* SuperGlue.forward (:207-276).  Outputs: matches0 [b][n0] / matches1 [b][n1] int64 (-1 where invalid),
 * matching_scores0 / 1 fp32.  z_out (nullable): [b][n0+1][n1+1], the log transport plan after
 * `Z - norm` (:170), for tests.  sinkhorn_iters >= 0. */
int sg_forward(const float* packed, int n_layers, const int32_t* layer_kinds, int sinkhorn_iters, float match_threshold,
               const float* kpts0, const float* scores0, const float* desc0,
               const float* kpts1, const float* scores1, const float* desc1,
               int b, int n0, int n1, int h0, int w0, int h1, int w1,
               int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* z_out,
               void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* Stage: keypoint normalisation (:62-69, image sizes h x w) + KeypointEncoder (:72-82, BatchNorm with running
 * statistics) added to the descriptors (:237-238): out_s = desc_s + kenc(normalize(kpts_s), scores_s). */
int sg_keypoint_encode(const float* packed, int n_layers,
                       const float* kpts0, const float* scores0, const float* desc0,
                       const float* kpts1, const float* scores1, const float* desc1,
                       int b, int n0, int n1, int h0, int w0, int h1, int w1, float* out0, float* out1,
                       void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* Stage: one step of AttentionalGNN.forward (:127-133) with GNN layer `layer` of kind `kind`: both sides'
 * deltas from the pre-update descriptors, out_s = desc_s + AttentionalPropagation(desc_s, source_s) (:111-124). */
int sg_layer(const float* packed, int n_layers, int layer, int kind, const float* desc0, const float* desc1,
             int b, int n0, int n1, float* out0, float* out1, void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* Stage: the softmax attention of MultiHeadedAttention (:85-88, :100-106) on given projections, the kernel sg_layer
 * and sg_forward run with the same launch shape: per batch item and head h (channels h*64 .. h*64+63),
 * out[h*64+d][n] = sum_m softmax_m(sum_e q[h*64+e][n] k[h*64+e][m] / 8) v[h*64+d][m].
 * Head-contiguous layout (the packed layout above): q [b][256][N], kv [b][512][M] (k rows 0..255, then v rows
 * 256..511), out [b][256][N].  N, M >= 1; out must not alias q or kv. */
int sg_attention(const float* q, const float* kv, int b, int N, int M, float* out, sg_stream_t stream);

/* Stage: log_optimal_transport (:148-170) on given scores [b][n0][n1] (already divided by sqrt(256))
 * with the dustbin score *bin_score (device) -> z_out [b][n0+1][n1+1]. */
int sg_sinkhorn(const float* scores, const float* bin_score, int b, int n0, int n1, int iters, float* z_out,
                void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* Stage: the match tail (:252-276) on a given z [b][n0+1][n1+1]: max / argmax of z[:-1, :-1] along rows and
 * columns (first index wins on exact ties), mutual check, exp, threshold. */
int sg_match_tail(const float* z, int b, int n0, int n1, float match_threshold, int64_t* matches0, int64_t* matches1,
                  float* mscores0, float* mscores1, void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* ---- Ragged batch (sg_version() >= 2): b pairs, each with its own n0[i], n1[i] and image sizes, in one chain of launches.
 *
 * Inputs are padded to the capacities cap0 / cap1: keypoints [b][cap][2], scores [b][cap], descriptors [b][256][cap].
 * n0, n1 ([b]) and hw0, hw1 ([b][2], (h, w) per item) are HOST int32 arrays, like layer_kinds; they travel to the kernels by
 * value, so the library still allocates nothing, copies nothing from host memory and never synchronises.
 *   - 1 <= b <= SG_MAX_ITEMS, and every item has 1 <= n0[i] <= cap0 and 1 <= n1[i] <= cap1 (an item with an empty side
 *     is the caller's to answer, as for sg_forward).
 *   - Nothing past an item's counts is read: padded input entries and stale workspace contents may hold anything.
 *   - Outputs matches0 / mscores0 [b][cap0], matches1 / mscores1 [b][cap1]; entries past an item's count are -1 / 0.f.
 *   - In z_out ([b][cap0+1][cap1+1]) item i occupies rows 0..n0[i] and columns 0..n1[i] of its slot at row stride cap1 + 1
 *     (the dustbin row is row n0[i], the dustbin column is column n1[i]); in a scores input ([b][cap0][cap1]) rows
 *     0..n0[i]-1 and columns 0..n1[i]-1 at row stride cap1.  The rest of a slot is unspecified.
 *   - Every item's outputs are bitwise those of the same pair run alone through the uniform entry points: the order of every
 *     reduction depends on the item's own counts, never on the capacities or on the other items.
 *   - All argument validation happens before the first HIP call: a bad argument returns -1 (a short workspace -2) with a
 *     message, also on a machine without a GPU.
 * sg_ragged_workspace_bytes returns 0 for a shape it refuses. */
size_t sg_ragged_workspace_bytes(int b, int cap0, int cap1);

int sg_forward_ragged(const float* packed, int n_layers, const int32_t* layer_kinds, int sinkhorn_iters, float match_threshold,
                      const float* kpts0, const float* scores0, const float* desc0,
                      const float* kpts1, const float* scores1, const float* desc1,
                      int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1, const int32_t* hw0, const int32_t* hw1,
                      int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1, float* z_out,
                      void* workspace, size_t workspace_bytes, sg_stream_t stream);

/* Ragged stages, for tests: sg_attention (q [b][256][capN], kv [b][512][capM], n / m HOST [b]), sg_sinkhorn and sg_match_tail. */
int sg_attention_ragged(const float* q, const float* kv, int b, int capN, int capM, const int32_t* n, const int32_t* m,
                        float* out, sg_stream_t stream);
int sg_sinkhorn_ragged(const float* scores, const float* bin_score, int b, int cap0, int cap1, const int32_t* n0,
                       const int32_t* n1, int iters, float* z_out, void* workspace, size_t workspace_bytes, sg_stream_t stream);
int sg_match_tail_ragged(const float* z, int b, int cap0, int cap1, const int32_t* n0, const int32_t* n1, float match_threshold,
                         int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                         void* workspace, size_t workspace_bytes, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
