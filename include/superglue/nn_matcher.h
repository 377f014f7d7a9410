/*
 * C ABI of the MI355X (gfx950) nearest-neighbour matcher, part of libsuperglue_hip.so (sg_version() >= 3).
 *
 * Replaces, on the GPU, the forward of the reference module
 *   src/models/matchers/nn/nearest_neighbour.py:41-63  (NearestNeighbour.forward)
 * with its helpers find_nn (:5-15) and mutual_check (:18-23): descriptor similarity, the two nearest neighbours
 * of every point in both directions, ratio test, distance test, mutual check.
 *
 * The n0 x n1 similarity matrix is never written: one kernel multiplies a 128 x 64 tile on v_mfma_f32_32x32x2_f32
 * (K = 256) and reduces it, in its epilogue, to {best, second, index of the best} per row and per column of the
 * tile; a second kernel merges those partials in ascending tile order and applies the tests.  No floating-point
 * atomics: two calls on the same inputs are bitwise identical.
 *
 * Conventions (superglue.h): every pointer is a DEVICE pointer to contiguous data unless stated otherwise (the
 * workspace 16-byte aligned, the others aligned to their element: a row of a larger buffer will do); all work is enqueued on `stream`; the library never allocates and never synchronises; functions
 * return 0 or a negative code (-1 bad argument, -2 workspace too small, -3 launch failed) with text from
 * sg_last_error(); every argument is validated on the host before the first launch.  Arithmetic is fp32.
 *
 * Shapes: descriptors [b][256][n] (channel-major, as SuperPoint emits them).  Outputs: matches0 [b][n0] /
 * matches1 [b][n1] int64 (-1 where a test fails), matching_scores0 / 1 fp32.
 *
 * Selection rules:
 *   - a column (row) is valid by its INDEX (< n1, < n0), never by its value: the zero padding of a tile has
 *     similarity 0, which beats every real similarity when all of those are negative;
 *   - on exactly equal similarities the lowest index wins (torch.topk leaves it unspecified);
 *   - the second value is the second of the multiset: a duplicated maximum gives second == best, as topk(2) does.
 * Tests, in the reference's fp32 arithmetic: dist = 2 * (1 - sim); with ratio > 0, dist0 <= (float)(ratio^2) * dist1;
 * with distance > 0, dist0 <= (float)(distance^2); score = (sim0 + 1) / 2 where the tests hold, 0 elsewhere.
 * ratio == 0 / distance == 0 switch a test off (the reference's `if ratio_thresh:`).  mutual != 0 rewrites matches0
 * only (matches0[i] survives iff matches1[matches0[i]] == i): matches1 and both score vectors are not touched by
 * it -- the reference as written.
 * Descriptors are expected finite; with NaN / infinite descriptors the matches are unspecified but stay in range.
 *
 * Refused (-1): b < 1, a side with no point; a ratio test with fewer than 2 points on either side (topk(2) raises
 * in the reference); negative or NaN thresholds; any bit of `flags`; outputs that overlap each other, the inputs
 * or the workspace; misaligned pointers.
 */
#ifndef ONEPOSE_AMD_NN_MATCHER_H
#define ONEPOSE_AMD_NN_MATCHER_H

#include "superglue.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NNM_DESC_DIM 256
#define NNM_MAX_ITEMS 64 /* items of one call, uniform or ragged */
#define NNM_TILE_ROWS 128 /* rows (side 0) of a similarity tile */
#define NNM_TILE_COLS 64  /* columns (side 1) of a similarity tile */
#define NNM_MAX_POINTS 65536

/* Bytes of workspace for b items of up to cap0 x cap1 points: the two zero-padded descriptor planes and the row /
 * column partials.  0 for a shape the entry points refuse. */
size_t nnm_workspace_bytes(int b, int cap0, int cap1);

/* The uniform batch: b pairs of n0 x n1 points. */
int nnm_match(const float* desc0, const float* desc1, int b, int n0, int n1, double ratio, double distance, int mutual,
              int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
              void* workspace, size_t workspace_bytes, sg_stream_t stream, int flags);

/* The ragged batch: 1 <= b <= NNM_MAX_ITEMS pairs in one chain of launches.  desc0 [b][256][cap0]; desc1
 * [b][256][cap1] or, with shared1 != 0, ONE plane [256][cap1] that every item reads (the detector's query frame).
 * n0, n1 are HOST int32 arrays [b] with 1 <= n0[i] <= cap0, 1 <= n1[i] <= cap1; they travel to the kernels by value.
 * Nothing past an item's counts reaches its results: padded input entries and stale workspace contents may hold
 * anything.  Outputs [b][cap0] / [b][cap1]; entries past an item's count are -1 / 0.f.  Tiles past an item's counts
 * return at once.  Every item's outputs are bitwise those of nnm_match on that pair alone. */
int nnm_match_ragged(const float* desc0, const float* desc1, const int32_t* n0, const int32_t* n1, int b, int cap0, int cap1,
                     int shared1, double ratio, double distance, int mutual,
                     int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                     void* workspace, size_t workspace_bytes, sg_stream_t stream, int flags);

/* Stage, for tests: the pack and the main loop of nnm_match on one pair, with the tile written out instead of
 * reduced: sim_out [n0][n1] = desc0^T desc1.  Workspace: nnm_workspace_bytes(1, n0, n1). */
int nnm_similarity(const float* desc0, const float* desc1, int n0, int n1, float* sim_out,
                   void* workspace, size_t workspace_bytes, sg_stream_t stream, int flags);

#ifdef __cplusplus
}
#endif
#endif
