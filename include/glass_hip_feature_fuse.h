/*
 * glass_hip_feature_fuse.h — entry points of libglass_hip.so (gfx950): the detections of several rotated and rescaled views of
 * one image fused into one detection set in the image's frame (test-time augmentation).
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_FUSE_H
#define GLASS_HIP_FEATURE_FUSE_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ fused views of one image
 * The model reads a word well only when it meets it roughly upright and at a workable size, so an image runs through it as V
 * views - rotations (glass_rotate_u8) at several scales.  glass_fuse_views turns their padded detections into ONE detection set
 * in the image's frame on the device.  It differs from glass_merge_views (glass_hip_ext_views.h) in four ways: the frame is a
 * full affine map; the copy of a word that is kept is the one with the best KEY, which may be the word score (the upside-down
 * copy of a word is detected as well as the upright one, but read badly); every survivor carries the set of views that found
 * it, the main false-positive filter of a multi-view run; and the per-view filter is one bounds rectangle on the centre, which
 * removes the detections in the fill corners of a rotated canvas.
 *   boxes [V,K,5] (cx, cy, w, h, angle in degrees) in the view's own pixels, scores [V,K], counts [V] ints;
 *   text_arg [V,K,T] ints and text_max [V,K,T] floats: what glass_text_argmax writes (both may be null when rank_mode == 0);
 *   view_affine [V,8] doubles ON THE DEVICE: m0..m5, s, dtheta - the matrix maps a view pixel to an image pixel, s is image
 *   pixels per view pixel, dtheta the degrees to add to a box angle;  bounds [4]: x0, y0, x1, y1 in the image's frame, a side
 *   may be -inf / +inf.
 * Semantics, in this order:
 *  1. Candidates.  Slot s of view v is a candidate for s < min(max(counts[v], 0), K); it is dropped if its score or any of
 *     its five box values is not finite.
 *  2. Key.  ws is the word score by the arithmetic of glass_postprocess_words: a float32 product, in step order, of
 *     text_max[v,s,t] for t = 0 .. up to and including the first step whose text_arg equals stop_index, or all T steps if
 *     there is none - bit for bit the text_score the word post-processor gives the slot.  rank_mode 0: key = score; 1: key =
 *     score * ws (one float32 product); 2: key = ws.  A key that is not finite drops the candidate.
 *  3. Frame.  The arithmetic of glass_rotate_boxes: every value widened to float64, every product and sum rounded on its own
 *     (no fused multiply-add):  gx = m0*cx + m1*cy + m2,  gy = m3*cx + m4*cy + m5,  gw = w*s,  gh = h*s,  a' = a + dtheta,
 *     then a' - 360*floor((a' + 180)/360); each rounded to float32 once.  The candidate is dropped unless all five are finite,
 *     gw > 0, gh > 0, x0 <= gx <= x1 and y0 <= gy <= y1 (tested on the float32 values).
 *  4. Order.  Key descending, ties by view ascending, then slot ascending (-0.0 and +0.0 are one key).
 *  5. Greedy cross-view pass.  Going through the order, a candidate is KEPT iff no earlier kept candidate of a DIFFERENT view
 *     has rotated IoU >= nms_thresh with it - the IoU function and the `>=` of glass_merge_views; pairs of one view are never
 *     compared.  A candidate that is not kept becomes a SUPPORTER of the earliest such kept candidate in the order.  The walk
 *     covers all candidates; it stops early only right after the candidate that takes the 1024th kept place, and the
 *     candidates after that one are neither kept nor supporters.  cut = 1 iff any candidate remained then.
 *  6. Votes.  A kept candidate's view set is its own view plus the views of its supporters, a 64-bit mask with bit v for view
 *     v; votes is the number of bits set.
 *  7. Output.  The kept candidates with votes >= min_votes, in order, n of them; the first min(n, max_out) are written:
 *     out_boxes [max_out,5] the boxes of step 3, out_scores [max_out] the detection scores, out_keys [max_out], out_src
 *     [max_out] = v*K + s, out_votes [max_out], out_views [max_out] the masks.  out_count[0] is the number of rows,
 *     out_count[1] is 1 iff cut or n > max_out, out_count[2] the number kept before the vote filter.  Rows beyond
 *     out_count[0] are left as the caller filled them.
 * Needs 0 <= V <= 64, 1 <= K <= 1024, V*K <= 8192, rank_mode in 0..2, stop_index >= 0, 1 <= T <= 64 when rank_mode != 0,
 * 1 <= min_votes <= 64, 1 <= max_out <= 1024, a finite nms_thresh, non-null pointers (the text arrays only when rank_mode != 0)
 * and `workspace` (16-byte aligned) >= glass_fuse_views_workspace_bytes(V, K); anything else returns a negative GLASS_E* code
 * with a message before any launch (the workspace query returns the code for a V, K outside the limits).  V == 0 writes
 * out_count = {0, 0, 0} and returns GLASS_OK.  view_affine is on the device, so the host cannot check it: a non-finite entry
 * drops that view's candidates in step 3.  Nothing read from `counts`, `text_arg` or the sort keys is used as an index
 * unchecked.  One launch of one workgroup (16 wave64; the sort keys, the kept boxes with their source slots and view masks
 * and the current chunk of 64 candidates live in LDS, the candidates' boxes and keys in the workspace; the output is one
 * ordered compaction after the walk), bounded loops, integer atomics only, no host synchronisation: results are bit-identical
 * from run to run.                                                                                                          */
int64_t glass_fuse_views_workspace_bytes(int V, int K);
int glass_fuse_views(const float* boxes, const float* scores, const int* counts, const int* text_arg, const float* text_max,
                     int T, int stop_index, int rank_mode, const double* view_affine, const float* bounds, int V, int K,
                     float nms_thresh, int min_votes, int max_out, float* out_boxes, float* out_scores, float* out_keys,
                     int* out_src, int* out_votes, int64_t* out_views, int* out_count, void* workspace,
                     int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_FUSE_H */
