/*
 * glass_hip_feature_chars.h — entry points of libglass_hip.so (gfx950): where inside its box every character of a word lies.
 *
 * One header per feature (see glass_hip_feature_roimask.h): it includes glass_hip.h, the binding parses it
 * (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers, ints for sizes, 0 or a negative GLASS_E*
 * code (glass_last_error() has the message), all work enqueued on the caller's stream, nothing synchronises.
 * glass_abi_version() does not change.
 *
 * Three stages: the attention rows of a forced replay of the emitted symbols (glass_forced_attention), the rows turned into
 * normalised spans along the width of the box the recogniser pooled (glass_char_spans), and the spans turned into quads in the
 * image (glass_char_quads).  The spans are normalised, so they survive every rescaling of the box; the quads are made last.
 */
#ifndef GLASS_HIP_FEATURE_CHARS_H
#define GLASS_HIP_FEATURE_CHARS_H

#include "glass_hip.h" /* glass_stream_t, glass_decoder_weights, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ the attention rows of a forced replay
 * glass_forced_decode (glass_hip.h) with one more output: out_attention float [B][n][L][T], L = max_len.  Every step of the
 * attention-GRU decoder forms a softmax over the T encoder positions of the item; these are the weights, which the decoder
 * kernels otherwise keep in LDS for one step only.
 *
 * Row t of a sequence holds the attention weights that formed the context vector of step t: the GRU input of step t is
 * [emb(y_{t-1}) | alpha_t . x], with y_{-1} = [GO].  Row 0 comes from the step -1 launch (h = 0, so it is the same for the n
 * sequences of an item); row t + 1 comes from the launch of step t.  Rows from the sequence's effective length on are zero:
 * the output is cleared by a memset (no launch) and a row is written only while its sequence goes on.  The effective length is
 * the one glass_forced_decode computes (from `lengths`, or up to and including the first `eos`); a sequence that stops at a
 * symbol outside [0, C) keeps the rows it computed before it.  A live row is non-negative and sums to 1 up to float32
 * rounding (a softmax: exp(e - max) / sum).
 *
 * Every other output (step_logp, scores, lengths, probs, logits) is what glass_forced_decode writes, bit for bit: the step
 * kernel is the same template, and the copy of the rows happens after the attention part has finished with them.
 * Same workspace as glass_forced_decode (glass_forced_attention_workspace_bytes returns the same number), still
 * 2 * max_len + 1 launches, no host synchronisation, bit-identical from run to run (a row has one writer, no atomics).
 * Limits as glass_forced_decode: D = 256, 1 <= T <= 64, 1 <= C <= 256, 1 <= n <= 16, 1 <= max_len <= 64, B >= 0; B == 0
 * launches nothing.  A null out_attention is GLASS_EINVAL.                                                                  */
int64_t glass_forced_attention_workspace_bytes(int B, int n, int T, int D, int C, int max_len);
int glass_forced_attention(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int n, int T, int D, int C,
                           int max_len, int eos, const int* targets, const int* lengths, float* out_step_logp,
                           float* out_scores, int* out_lengths, float* out_probs, float* out_logits, float* out_attention,
                           void* workspace, int64_t workspace_bytes, glass_stream_t stream);

/* ------------------------------------------------------------------ attention rows -> spans along the box
 * The statement is glass_amd.postprocess.char_boxes.char_spans_host (numpy float64).  Every input value is widened exactly to
 * float64 and every formula is evaluated in float64, without contraction; the results are rounded to float32 once.
 *
 * Input: attention float [R][L][T], targets int32 [R][L], lengths int32 [R], eos.  For word r: len = min(max(lengths[r], 0), L);
 * m, the number of character steps, is len - 1 if len > 0 and targets[r][len - 1] == eos, else len.  A symbol is compared
 * with eos and never used as an index.  Rows from m on are never read.
 *
 * Encoder column j lies at p_j = (j + 0.5) / T of the box's width.  For t < m:
 *   S_t = sum_j a_tj;  centre c_t = sum_j a_tj p_j / S_t;  spread s_t = sqrt(sum_j a_tj (p_j - c_t)^2 / S_t).
 * The three sums are taken over the 64 lanes of a wavefront by a fixed butterfly (lanes >= T add 0), so they may differ from a
 * sequential sum in the last bits of the float64 - far below the one float32 rounding of the outputs.
 * If S_t is not finite or <= 0, or any a of the row is negative or not finite, the WORD is invalid: count = 0, all its outputs
 * zero, valid = 0.  Its neighbours are untouched.
 * Boundaries: b_t = (c_t + c_{t+1}) / 2 for t < m - 1.  The outer edges are mirrored and clamped to [0, 1]:
 *   e_L = c_0 - |b_0 - c_0|,  e_R = c_{m-1} + |c_{m-1} - b_{m-2}|;  for m = 1 the span is (0, 1).
 * Span of step t: (min(l, r), max(l, r)) with l = b_{t-1} (t = 0: e_L) and r = b_t (t = m - 1: e_R).
 * monotone = 1 iff the centres are strictly increasing (m <= 1: 1).  Attention need not be monotone: the spans are defined by
 * the rule above all the same, and the flag is the quality signal a caller filters on.
 *
 * Outputs, all zero from row m on, every element written whatever the inputs (no initialisation needed):
 *   spans float [R][L][2], centres float [R][L], spreads float [R][L], count, monotone, valid int32 [R] (count = m, or 0 for
 *   an invalid word; a word with m = 0 is valid and monotone).
 * One wavefront per word, a lane per column, the steps in a loop; the m centres stay in LDS for the boundaries.  One launch;
 * R == 0 returns without one.  Needs R >= 0, 1 <= L <= 64, 1 <= T <= 64 and non-null pointers (R > 0).  Deterministic.      */
int glass_char_spans(const float* attention, const int* targets, const int* lengths, int R, int L, int T, int eos, float* spans,
                     float* centres, float* spreads, int* count, int* monotone, int* valid, glass_stream_t stream);

/* ------------------------------------------------------------------ spans -> quads in the image
 * Input: spans float [R][L][2], count int32 [R], frames float [R][5] = (cx, cy, w, h, angle in degrees) - the box the
 * recogniser pooled, in the pixels the quads are wanted in.  Output: quads float [R][L][4][2], rows from min(max(count, 0), L)
 * on zero, every element written.
 *
 * The frame convention is the recogniser pooler's own (csrc/roi_align.hip): with t = angle * pi / 180 the width runs along
 * u = (cos t, -sin t) and the height along v = (sin t, cos t).  The rectangle of a span (lo, hi) has centre
 * (cx, cy) + ((lo + hi) / 2 - 0.5) * w * u, extents ((hi - lo) * w, h) and the frame's angle; its corners come in the order
 * PostProcessorRotatedBoxes.boxes_to_polygons emits for a box: centre -eu -fv, +eu -fv, +eu +fv, -eu +fv with e, f the half
 * extents - so a span (0, 1) gives the word's own polygon.  Arithmetic in float64, rounded to float32 once.
 * A frame with a non-finite component or w <= 0 or h <= 0 gives zero rows.
 * One launch; R == 0 returns without one.  Needs R >= 0, 1 <= L <= 64 and non-null pointers (R > 0).                       */
int glass_char_quads(const float* spans, const int* count, const float* frames, int R, int L, float* quads, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_CHARS_H */
