/*
 * glass_hip_feature_lines.h — entry points of libglass_hip.so (gfx950): detected words grouped into text lines in reading order.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_LINES_H
#define GLASS_HIP_FEATURE_LINES_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ line grouping
 * The statement is glass_amd.postprocess.line_grouping.group_lines_host (numpy float64), which the kernels equal in every
 * integer output wherever no comparison falls within a few float64 ulps of its threshold.
 *
 * Input: boxes float [N][K][5], count int32 [N].  Image n has min(max(count[n], 0), K) words b_i = (cx, cy, w, h, a), a in
 * degrees, in the convention of box_polygon (csrc/postprocess_common.h).  Rows beyond the count are never read.  Every value
 * is widened exactly to float64 and every formula below is evaluated in float64.  With t = a * pi / 180,
 * u_i = (cos t, -sin t) is the reading direction and v_i = (sin t, cos t) the downward direction of the word.  A word is
 * valid if its five values are finite and w > 0, h > 0.
 *
 * Link(i, j), a symmetric pair rule: both words valid, i != j, and with d = c_j - c_i, H = max(h_i, h_j), h = min(h_i, h_j)
 *   1. |wrap(a_j - a_i)| <= max_angle_diff, wrap into [-180, 180), evaluated as r = fmod(|a_j - a_i|, 360), r > 180: 360 - r
 *      (the same bits for (i, j) and (j, i)).  Upside-down neighbours are NOT linked (unlike the merge step's mod-180 rule).
 *   2. h >= min_height_ratio * H
 *   3. |d.v_i| <= max_offset * H and |d.v_j| <= max_offset * H
 *   4. |d.u_i| - (w_i + w_j) / 2 <= max_gap * H and the same with u_j; a negative gap (overlap) passes.
 * params double [4] on the HOST = max_angle_diff (0..180), min_height_ratio (0..1), max_offset (>= 0), max_gap (>= 0);
 * a non-finite, negative or out-of-range value returns GLASS_EINVAL before any launch.
 *
 * Lines: the connected components of Link.  An invalid word is a line of its own whose line box is its own five values
 * copied bit for bit; invalid words come after all valid lines, in index order.
 * Line frame: D = sum over the members of w_i u_i, summed in index order; U = D / |D| if |D| > 1e-12 * sum w_i, otherwise the
 *   u of the line's smallest-index word (a chain that closes a circle); V = (-U_y, U_x).
 * Order inside a line: ascending c_i.U, ties by index.
 * Line box: the four corners c_i +- (w_i / 2) u_i +- (h_i / 2) v_i of all members projected on U and V; the box is (centre,
 *   extent along U, extent along V, atan2(-U_y, U_x) in degrees), rounded to float32 once, at the end.
 * Order of lines: the page frame P_U, P_V is built the same way from all valid words (a fixed-shape tree sum; fallback
 *   (1, 0)); lines go ascending by m.P_V, then m.P_U, then smallest member index, m the unrounded box centre.  This is
 *   top-to-bottom and no more: two columns interleave row by row.  (POST_PROCESSING.ORDER_LINES, glass_hip_feature_layout.h,
 *   orders these lines column by column and cuts them into blocks; nothing here changes with it.)
 *
 * Outputs, every row written up to K whatever the count:
 *   line_id    int32 [N][K]      rank of the word's line, -1 from the count on
 *   line_pos   int32 [N][K]      position in the line, -1 from the count on
 *   order      int32 [N][K]      order[p] = word index, lines in rank order and words in position order, -1 beyond the count
 *   line_start int32 [N][K + 1]  CSR into order; entries from the line count on equal the count
 *   line_boxes float [N][K][5]   row l is line l, zeros beyond the line count
 *   line_count int32 [N]         number of lines
 *
 * Determinism: the link relation is 64-bit row words in the workspace (ceil(K / 64) words per row), written by one wavefront
 * per (image, 64-word row block); the components are found by hooking the larger label under the smaller with integer
 * minimum atomics in LDS until nothing changes, whose fixed point (every word labelled with its component's smallest index)
 * does not depend on the order of the atomics; every sum has a fixed order, there are no float atomics, and ranks are counts
 * of smaller keys.  Two runs are bit-identical, and an image's result does not depend on its neighbours in the batch.
 * Nothing read from memory is used as an index unchecked.
 *
 * glass_group_lines_workspace_bytes: bytes of the workspace (16-byte aligned, needs no initialisation); negative for bad sizes.
 * glass_group_lines: needs N >= 0, 0 <= K <= GLASS_GROUP_LINES_MAX_K and non-null pointers (boxes and the [N][K] outputs may
 *   be null when K == 0); anything else returns a negative code before any launch.  N == 0 launches nothing.  Two launches
 *   (one when K == 0).                                                                                                      */
#define GLASS_GROUP_LINES_MAX_K 1024
int64_t glass_group_lines_workspace_bytes(int N, int K);
int glass_group_lines(const float* boxes, const int* count, int N, int K, const double* params4_host, int* line_id,
                      int* line_pos, int* order, int* line_start, float* line_boxes, int* line_count, void* workspace,
                      int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_LINES_H */
