/*
 * glass_hip_feature_layout.h — entry points of libglass_hip.so (gfx950): text lines ordered column by column and cut into blocks.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_LAYOUT_H
#define GLASS_HIP_FEATURE_LAYOUT_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ page order and blocks
 * The statement is glass_amd.postprocess.line_order.order_lines_host (numpy float64), which the kernels equal in every integer
 * output wherever no comparison falls within a few float64 ulps of its threshold.  The order is the classical one for OCR
 * output: two ordering rules between pairs of lines (Breuel) and a topological sort, made deterministic by a key.
 *
 * Input: line_boxes float [N][K][5] and line_count int32 [N] as the line grouper of glass_hip_feature_lines.h writes them, and
 * optionally line_start int32 [N][K + 1] (may be null).  Image n has L = min(max(line_count[n], 0), K) lines, K <= 1024.  Rows
 * from L on are never read.  Every value is widened exactly to float64 and every formula below is evaluated in float64
 * without contraction; there are no float atomics.
 *
 * Geometry.  A line (cx, cy, w, h, a) is valid iff its five values are finite and w > 0, h > 0.  With t = a * pi / 180,
 * u_l = (cos t, -sin t) and v_l = (sin t, cos t).  Page frame: D = sum of w_l u_l over the valid lines, a fixed-shape tree sum
 * over 1024 slots (slot i + slot i + stride, stride halving from 512; zeros where there is no valid line); P_U = D / |D| if
 * |D| > 1e-12 * sum w_l, otherwise (1, 0); P_V = (-P_U.y, P_U.x).  For a valid line the four corners
 * c +- (w / 2) u +- (h / 2) v projected on P_U and P_V give [ulo, uhi] and [vlo, vhi]; mu = c.P_U, mv = c.P_V; its key is
 * (mv, mu, index).
 *
 * Relations between two valid lines a != b:
 *   over(a, b), symmetric: min(uhi_a, uhi_b) - max(ulo_a, ulo_b) > min_overlap * min(uhi_a - ulo_a, uhi_b - ulo_b).
 *   Rule 1: over(a, b) and mv_a < mv_b: a precedes b.
 *   Rule 2: not over(a, b), mu_a < mu_b, and there is no valid c other than a, b with over(c, a), over(c, b) and
 *           min(mv_a, mv_b) < mv_c < max(mv_a, mv_b): a precedes b.
 *   Equal mv under rule 1, or equal mu under rule 2, gives no edge.
 *
 * Order.  Repeat until every valid line is emitted: a line is ready if none of its predecessors is un-emitted; emit the ready
 * line with the smallest key; if no line is ready (a cycle), emit the un-emitted line with the smallest key and add 1 to
 * `forced`.  The invalid lines follow all valid ones, in index order.
 *
 * Blocks.  The order is cut into maximal runs.  Consecutive valid lines p, q stay in one block iff over(p, q), mv_p < mv_q,
 * vlo_q - vhi_p <= block_max_gap * max(h_p, h_q) (a negative gap passes) and min(h_p, h_q) >= block_min_height_ratio *
 * max(h_p, h_q), h the line box's own height.  A block's box is its members' corners enclosed in the page frame: (centre,
 * extent along P_U, extent along P_V, atan2(-P_U.y, P_U.x) in degrees), rounded to float32 once, at the end.  An invalid
 * line is a block of its own whose box is its five values copied bit for bit.
 *
 * params double [3] on the HOST = min_overlap in [0, 1), block_max_gap >= 0, block_min_height_ratio in [0, 1]; a non-finite
 * or out-of-range value returns GLASS_EINVAL before any launch.
 *
 * Outputs, every row written up to K whatever the count:
 *   page_rank   int32 [N][K]      position of the line in the order, -1 from L on
 *   page_order  int32 [N][K]      the inverse of page_rank, -1 beyond
 *   block_id    int32 [N][K]      per line, -1 from L on
 *   block_start int32 [N][K + 1]  CSR into page_order; entries from the block count on equal L
 *   block_boxes float [N][K][5]   zeros beyond the block count
 *   block_count int32 [N]         number of blocks
 *   forced      int32 [N]         number of forced emissions
 *   line_first  int32 [N][K]      only when line_start is given (null otherwise): the number of words in the lines ahead of this
 *                                 line in the order, so a word's page rank is line_first[line] + line_pos; -1 from L on.  A
 *                                 line_start entry outside [0, K] or a decreasing pair makes the line's size 0.
 *
 * Known limits.  Two pieces of one row that the line grouper left apart (a table) read column by column.  L-shaped regions
 * and text at angles far from the page's follow the rules, not a human.
 *
 * Determinism: every line's rank by key is a count of smaller keys, and all later matrices are indexed by that rank, so "mv
 * strictly between" is a range of ranks (equal-mv runs excluded by per-line run bounds).  The relations are 64-bit row
 * words in the workspace written by one wavefront per (image, 64-row block) by ballot; in-degrees are integer sums in a
 * fixed order; the emission is an integer minimum per step.  Every sum has a fixed order and there are no float atomics.
 * Two runs are bit-identical, and an image's result does not depend on its neighbours in the batch.  Nothing read from
 * memory is used as an index unchecked.  Every loop is bounded: the emission loop runs exactly L times.
 *
 * glass_order_lines_workspace_bytes: bytes of the workspace (16-byte aligned, needs no initialisation); negative for bad sizes.
 * glass_order_lines: needs N >= 0, 0 <= K <= GLASS_ORDER_LINES_MAX_K and non-null pointers (line_boxes and the [N][K] outputs
 *   may be null when K == 0; line_start and line_first are both null or both given); anything else returns a negative code
 *   before any launch.  N == 0 launches nothing.  Four launches (one when K == 0).                                         */
#define GLASS_ORDER_LINES_MAX_K 1024
int64_t glass_order_lines_workspace_bytes(int N, int K);
int glass_order_lines(const float* line_boxes, const int* line_count, const int* line_start, int N, int K,
                      const double* params3_host, int* page_rank, int* page_order, int* block_id, int* block_start,
                      float* block_boxes, int* block_count, int* forced, int* line_first, void* workspace,
                      int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_LAYOUT_H */
