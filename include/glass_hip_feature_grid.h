/*
 * glass_hip_feature_grid.h — entry points of libglass_hip.so (gfx950): text lines aligned into rows, cells, tables and columns.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_GRID_H
#define GLASS_HIP_FEATURE_GRID_H

#include "glass_hip.h" /* glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ rows, cells, tables and columns
 * The statement is glass_amd.postprocess.row_grid.row_grid_host (numpy float64), which the kernels equal in every integer
 * output wherever no comparison falls within a few float64 ulps of its threshold.  The page order of
 * glass_hip_feature_layout.h reads two pieces of one row that the line grouper left apart column by column; this feature
 * keeps them together: the item of a receipt with its amount, the cells of a table row with each other.
 *
 * Input: line_boxes float [N][K][5] and line_count int32 [N] as the line grouper of glass_hip_feature_lines.h writes them, and
 * optionally line_start int32 [N][K + 1] (may be null).  Image n has L = min(max(line_count[n], 0), K) lines, K <= 1024.  Rows
 * from L on are never read.  Every value is widened exactly to float64 and every formula below is evaluated in float64
 * without contraction; there are no float atomics.
 *
 * Geometry: the formulas of the page order (glass_hip_feature_layout.h), so the two features agree on every interval.  A
 * line (cx, cy, w, h, a) is valid iff its five values are finite and w > 0, h > 0.  With t = a * pi / 180,
 * u_l = (cos t, -sin t) and v_l = (sin t, cos t).  Page frame: D = sum of w_l u_l over the valid lines, a fixed-shape tree sum
 * over 1024 slots (slot i + slot i + stride, stride halving from 512; zeros where there is no valid line); P_U = D / |D| if
 * |D| > 1e-12 * sum w_l, otherwise (1, 0); P_V = (-P_U.y, P_U.x).  For a valid line the four corners
 * c +- (w / 2) u +- (h / 2) v projected on P_U and P_V give [ulo, uhi] and [vlo, vhi]; mu = c.P_U, mv = c.P_V; h is the line
 * box's own height.
 *
 * Relations between two valid lines a != b, all symmetric:
 *   beside(a, b):  min(uhi_a, uhi_b) - max(ulo_a, ulo_b) <= 0: disjoint along the text.
 *   rowmate(a, b): beside(a, b), min(vhi_a, vhi_b) - max(vlo_a, vlo_b) >= row_min_overlap * min(vhi_a - vlo_a, vhi_b - vlo_b)
 *                  and min(h_a, h_b) >= row_min_height_ratio * max(h_a, h_b).
 *   Rows are the connected components of rowmate; a row of at least two lines is multi-cell.
 *   over(a, b):    min(uhi_a, uhi_b) - max(ulo_a, ulo_b) > column_min_overlap * min(uhi_a - ulo_a, uhi_b - ulo_b).
 *   colmate(a, b): both lines lie in multi-cell rows, the two rows are different, over(a, b), and
 *                  max(vlo_a, vlo_b) - min(vhi_a, vhi_b) <= table_max_row_gap * max(h_a, h_b) (a negative gap passes).
 *   Columns are the connected components of colmate; tables are the connected components of rowmate and colmate together,
 *   both among the lines of multi-cell rows.  A line of a single-line row, and an invalid line, belongs to no table and no
 *   column (-1).
 *
 * Numbering.  Every key is a total order, so each number is a count of smaller keys.  Rows by (smallest mv among their
 * members, smallest member index); the invalid lines are rows of their own after all the others, in index order.  Cells
 * inside a row by (mu, index): row_pos.  Tables by their smallest row id.  Columns inside their table by (smallest ulo among
 * their members, smallest member index).  Two lines of one row may share a column and a column may lack a line in some row:
 * both are legal and carried as they are.
 *
 * Boxes.  A row's and a table's box is its members' corners enclosed in the page frame: (centre, extent along P_U, extent
 * along P_V, atan2(-P_U.y, P_U.x) in degrees), rounded to float32 once, at the end.  An invalid line's row box is its five
 * values copied bit for bit.
 *
 * params double [4] on the HOST = row_min_overlap in (0, 1], row_min_height_ratio in [0, 1], column_min_overlap in [0, 1),
 * table_max_row_gap >= 0; a non-finite or out-of-range value returns GLASS_EINVAL before any launch.
 *
 * Outputs, every row written up to K whatever the count, -1 meaning "none":
 *   row_id      int32 [N][K]      the line's row, -1 from L on
 *   row_pos     int32 [N][K]      the line's cell number inside its row, -1 from L on
 *   table_id    int32 [N][K]      the line's table, -1 where it has none and from L on
 *   col_id      int32 [N][K]      the line's column inside its table, -1 where it has none and from L on
 *   row_order   int32 [N][K]      the lines row by row, cells in row_pos order, -1 from L on
 *   row_start   int32 [N][K + 1]  CSR into row_order; entries from the row count on equal L
 *   row_boxes   float [N][K][5]   zeros beyond the row count
 *   row_count   int32 [N]
 *   table_boxes float [N][K][5]   zeros beyond the table count
 *   table_rows  int32 [N][K]      rows per table, 0 beyond the table count
 *   table_cols  int32 [N][K]      columns per table, 0 beyond the table count
 *   table_count int32 [N]
 *   row_first   int32 [N][K]      only when line_start is given (null otherwise): the number of words in the lines ahead of this
 *                                 line in row_order, so a word's row-major rank is row_first[line] + line_pos; -1 from L on.  A
 *                                 line_start entry outside [0, K] or a decreasing pair makes the line's size 0.
 *
 * Known limits.  Two prose columns whose lines stand at equal heights come out as rows: geometry alone cannot tell them from
 * a table, so the caller chooses the reading.  A cell of several lines is several rows.  A spanning cell inside a multi-cell
 * row joins the columns it covers.  Lines at angles far from the page's follow the rules, not a human.
 *
 * Determinism: the two pairwise relations are 64-bit row words in the workspace written by one wavefront per (image, 64-row
 * block) by ballot.  Each of the three sets of components is found by minimum-label propagation with hooking and a pointer
 * jump per round: a line's label is the smallest index it has heard of, a round reads only what the round before left and
 * combines by integer minimum, whose result does not depend on the order; the fixed point (every line labelled with the
 * smallest index of its component) is unique, the loop stops at the first round that changes nothing, and it is bounded by K
 * rounds, which a component of diameter K - 1 reaches even without the hooking and the jump.  Every number is an integer
 * count in a fixed order and every box a minimum and maximum in a fixed order; there are no float atomics.  Two runs are bit-identical, and an image's result does not depend on its neighbours in the batch.  Nothing read
 * from memory is used as an index unchecked.
 *
 * glass_row_grid_workspace_bytes: bytes of the workspace (16-byte aligned, needs no initialisation; 0 when N or K is 0, and
 *   the workspace may then be null); negative for bad sizes.
 * glass_row_grid: needs N >= 0, 0 <= K <= GLASS_ROW_GRID_MAX_K and non-null pointers (line_boxes and the [N][K] outputs may be
 *   null when K == 0; line_start and row_first are both null or both given); anything else returns a negative code before
 *   any launch.  N == 0 launches nothing.  Three launches (one when K == 0).                                              */
#define GLASS_ROW_GRID_MAX_K 1024
int64_t glass_row_grid_workspace_bytes(int N, int K);
int glass_row_grid(const float* line_boxes, const int* line_count, const int* line_start, int N, int K,
                   const double* params4_host, int* row_id, int* row_pos, int* table_id, int* col_id, int* row_order,
                   int* row_start, float* row_boxes, int* row_count, float* table_boxes, int* table_rows, int* table_cols,
                   int* table_count, int* row_first, void* workspace, int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_GRID_H */
