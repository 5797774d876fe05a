/*
 * glass_hip_feature_wdfa.h — entry points of libglass_hip.so (gfx950): beam search constrained by a WEIGHTED automaton.
 *
 * One header per feature (see glass_hip_feature_dfa.h): the earlier headers are closed, the binding parses every
 * include/glass_hip_feature_<feature>.h (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers,
 * ints for sizes, 0 or a negative GLASS_E* code (glass_last_error() has the message), all work enqueued on the caller's stream,
 * nothing synchronises.  glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_WDFA_H
#define GLASS_HIP_FEATURE_WDFA_H

#include "glass_hip.h" /* glass_decoder_weights, glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* one entry of the transition table: 8 bytes, 8-byte aligned, read with ONE 64-bit load per (beam, class) */
typedef struct {
  int32_t next; /* -1 = no transition, else the target state in bits 0..23 and min(dist[target], 127) in bits 24..30 */
  float w;      /* the transition's weight (a natural log); not finite = no transition */
} glass_wdfa_transition;

/* ------------------------------------------------------------------ beam search constrained by a weighted automaton
 * The pattern-constrained search of glass_hip_feature_dfa.h ("the DFA search" below) with a weight on every transition, every
 * stop and every start, added to the score the beams are RANKED by (shallow fusion: a character n-gram model crossed with the
 * pattern, word priors pushed toward the root of a trie, a length bonus -
 * glass_amd.evaluation.weighted_pattern.WeightedPattern builds the tables).  It is that
 * search element for element - fold, accept, start, item_pattern, the length rule t + 1 + dist <= L - 1, the stop rule, dead
 * slots, the range checks of states, fold symbols and segments, the limits - with these differences:
 *   trans [N][F] glass_wdfa_transition in the place of next;
 *   final_w [N] floats: the weight of stopping in state q;  start_w [S] floats: the weight a segment starts with;
 *   weight_scale: a kernel argument, so a caller sweeps it without rebuilding tables.
 * Every slot carries TWO float32 scores:
 *   the model score m: the running score plus the fp32 log-softmax, exactly the arithmetic (and the bits) of the unweighted
 *     searches;
 *   the weight sum a: start_w[segment] at the first step, + w for a symbol, + final_w[q] for the stop, one float32 addition
 *     per step, in step order.
 * A candidate's FUSED score is fmaf(weight_scale, a', m'): the product is not rounded on its own, ONE rounding gives the
 * result (so weight_scale = 0, or all-zero weights, give m' bit for bit).  Selection runs on the fused score with the rule of
 * the other searches: score descending, then flat index beam * C + class ascending, -inf last.  The finalisation ranks the
 * completed entries by fused score, then step, then slot.
 * A transition whose w is not finite counts as absent; so does a stop at a state whose final_w is not finite, a segment whose
 * start_w is not finite (a dead item), and any candidate whose weight sum a' is not finite: nothing is ranked by such a value.
 * Outputs as the DFA search's, with
 *   out_scores [B,k]: the fused scores;  out_model_scores [B,k]: m (-inf for an absent hypothesis, as out_scores);
 *   out_path_probs [B,max_len,C] (or null): from the MODEL scores, expf(m_t - m_{t-1}) at the emitted symbol - a row keeps
 *     meaning "the step's conditional probability", so every consumer of path rows is untouched.
 * Needs what the DFA search needs; B == 0 returns GLASS_OK.  `workspace` (16-byte aligned) >=
 * glass_beam_search_wdfa_workspace_bytes() = the DFA search's workspace + two [B][max_len][k] float tables (the weight sums,
 * the fused scores).  2 * max_len + 2 launches, ordinary grids with bounded loops, no host synchronisation, no
 * float atomics: results are bit-identical from run to run.                                                                  */
int64_t glass_beam_search_wdfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len);
int glass_beam_search_wdfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D, int C,
                           int max_len, int eos, const glass_wdfa_transition* trans, const float* final_w, const float* start_w,
                           const int* accept, const int* start, const int* fold, int N, int S, int F, const int* item_pattern,
                           float weight_scale, int* out_symbols, float* out_scores, float* out_model_scores, int* out_lengths,
                           int* out_tags, float* out_path_probs, void* workspace, int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_WDFA_H */
