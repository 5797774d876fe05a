/*
 * glass_hip_ext_views.h — entry points of libglass_hip.so (gfx950) for tiled inference: the cross-view merge.
 *
 * glass_hip.h and glass_hip_ext.h are both closed (the host tests pin their sets of prototypes).  From here on every feature
 * that adds entry points brings a header of its own, include/glass_hip_ext_<feature>.h, which includes glass_hip.h; the
 * binding parses every such header (glass_amd._lib.addon_signatures, ADDON_EXPORTS).  Same conventions as glass_hip.h: plain
 * C, raw device pointers, ints for sizes, every function returns 0 or a negative GLASS_E* code (glass_last_error() has the
 * message), all work is enqueued on the caller's stream, nothing synchronises unless stated.  The additions do not change
 * glass_abi_version(): a binding finds them by symbol.
 */
#ifndef GLASS_HIP_EXT_VIEWS_H
#define GLASS_HIP_EXT_VIEWS_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ merge of the views of one image (tiled inference)
 * A large image runs through the model as V views: overlapping tiles at full resolution and, for the words too large for a
 * tile, one low-resolution view of the whole image.  glass_merge_views turns their padded detections into ONE image's
 * detection set on the device: a word cut by a tile edge is dropped, a word seen whole by two or four tiles is kept once.
 *   boxes [V,K,5] (cx, cy, w, h, angle in degrees) in the view's own pixels, scores [V,K], counts [V] ints;
 *   view_xform [V,3]: ox, oy, inv - the view's origin in the image's frame and image pixels per view pixel;
 *   keep_rect [V,4]: kx0, ky0, kx1, ky1 in the image's frame, a side may be -inf / +inf;  size_range [V,2]: lo, hi.
 * Semantics, in this order:
 *  1. Candidates.  Slot s of view v is a candidate for s < min(max(counts[v], 0), K); it is dropped if its score or any of
 *     its five box values is not finite.
 *  2. Frame.  gx = cx*inv + ox, gy = cy*inv + oy, gw = w*inv, gh = h*inv, the angle unchanged: float32, every product and
 *     sum rounded separately (no fused multiply-add), so a float32 replay on the host gives the same bits.  The candidate is
 *     dropped unless gw > 0 and gh > 0.
 *  3. Border and size band.  The four corners of the global box are those of the rotated IoU (half extents cos/sin of
 *     angle * 0.01745329251 computed in double, rounded to float, times 0.5f; the corner sums in float32 without fused
 *     multiply-add); xmin..ymax are their extremes and size = max(xmax - xmin, ymax - ymin).  The candidate is kept iff
 *     kx0 <= xmin, xmax <= kx1, ky0 <= ymin, ymax <= ky1 and lo < size <= hi.
 *  4. Order.  Score descending, ties by view ascending, then slot ascending (-0.0 and +0.0 are one score).
 *  5. Greedy cross-view suppression.  Going through the order, a candidate is kept iff no EARLIER KEPT candidate of a
 *     DIFFERENT view has rotated IoU >= nms_thresh with it - the IoU function and the `>=` of glass_rotated_nms_select.
 *     Pairs of one view are never compared: the model's own NMS already judged them, and the word post-processor's merge
 *     step needs both halves of a split word.
 *  6. Output.  The first min(kept, max_out) kept candidates, in order: out_boxes [max_out,5] the global boxes of step 2,
 *     out_scores [max_out] copied, out_src [max_out] = v*K + s, out_count[0] their number.  out_count[1] is 1 iff, when the
 *     max_out-th candidate was kept, at least one candidate remained after it in the order (the output may be truncated);
 *     otherwise 0.  Rows beyond out_count[0] are left as the caller filled them.
 * Needs 0 <= V <= 256, 1 <= K <= 1024, V*K <= 8192 (the limit of glass_rotated_nms_select), 1 <= max_out <= 1024, a finite
 * nms_thresh, non-null pointers and `workspace` (16-byte aligned) >= glass_merge_views_workspace_bytes(V, K); anything else
 * returns a negative GLASS_E* code with a message before any launch (the workspace query returns the code for a V, K outside
 * the limits).  V == 0 writes out_count = {0, 0} and returns GLASS_OK.  Nothing read from `counts` is used as a bound
 * unclamped.  One launch of one workgroup (16 wave64; the sort keys, the kept boxes and the current chunk of 64 candidates live
 * in LDS, the candidates' global boxes in the workspace), bounded loops, no host synchronisation, no float atomics: results
 * are bit-identical from run to run.                                                                                        */
int64_t glass_merge_views_workspace_bytes(int V, int K);
int glass_merge_views(const float* boxes, const float* scores, const int* counts, const float* view_xform,
                      const float* keep_rect, const float* size_range, int V, int K, float nms_thresh, int max_out,
                      float* out_boxes, float* out_scores, int* out_src, int* out_count, void* workspace,
                      int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_EXT_VIEWS_H */
