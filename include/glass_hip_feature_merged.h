/*
 * glass_hip_feature_merged.h — entry points of libglass_hip.so (gfx950): constrained beam searches that MERGE the classes of
 * a fold symbol (case variants), so that a hypothesis is a string of fold symbols.
 *
 * One header per feature (see glass_hip_feature_dfa.h): the earlier headers are closed, the binding parses every
 * include/glass_hip_feature_<feature>.h (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers,
 * ints for sizes, 0 or a negative GLASS_E* code (glass_last_error() has the message), all work enqueued on the caller's stream,
 * nothing synchronises.  glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_MERGED_H
#define GLASS_HIP_FEATURE_MERGED_H

#include "glass_hip_feature_wdfa.h" /* glass_wdfa_transition; glass_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ fold-merged constrained beam searches
 * The pattern-constrained search of glass_hip_feature_dfa.h and the weighted one of glass_hip_feature_wdfa.h (the names here put
 * `merged` BEFORE dfa / wdfa: no entry of this header contains the name of an entry of those two) with one more stage in the
 * step: the candidates of a beam whose classes share a fold symbol become ONE candidate.  Everything else - tables, the
 * meaning of the mask, the length and stop rules, dead slots, selection rule, finalisation, outputs, limits, workspace, launch
 * count - is the unmerged search's, element for element.
 *
 * Groups.  fold[c] is the fold symbol of class c (-1 for the specials and the stop).  The GROUP of fold symbol f is the set of
 * classes whose fold is f, ascending, given as a CSR on the device:
 *   group_start [F + 1] ints, group_cls [n_group_cls] ints: the group of f is group_cls[group_start[f] .. group_start[f + 1]);
 *   1 <= n_group_cls <= C.  The caller guarantees: every class in at most one group, fold equal within a group, the stop in
 *   none (glass_amd.evaluation.pattern.DecodePattern.fold_groups builds them, ops.native validates hand-made ones).  The
 *   kernel range-checks every entry before it is used as an index; an entry outside its range is skipped.
 *
 * Semantics.  A hypothesis is a string of fold symbols.  At step t, for a live beam r with running model score run[r] and
 * every fold symbol f the constraint allows from r's state (its decision is per fold symbol, so it is the same for every
 * member of a group):
 *   ONE candidate per (r, f), in the place of the one-per-class candidates;
 *   its model score is the log of the group's summed mass: with c_i = run[r] + logp[r][i] over the group's classes i (the
 *     fp32 candidates of the unmerged search, bit for bit), M = max c_i and s = M + logf(sum_i expf(c_i - M)), in fp32 with
 *     the precise expf / logf, summed in ascending class order.  A member at -inf adds 0, a group that is all -inf gives
 *     -inf, a one-class group gives c_i bit for bit (no exp / log round trip);
 *   its emitted class is the group's arg-max, ties to the lowest class: the REPRESENTATIVE.  Its embedding feeds the next
 *     step, its class id goes into the symbol table, the output symbols and the path row - the text keeps the likeliest
 *     casing per position;
 *   the stop is never merged, nor is a class whose fold is outside [0, F).
 * Weighted search: weights are per fold symbol; the fused score is fmaf(weight_scale, a', s) with the merged s, and
 * out_model_scores carries s.
 *
 * Invariant.  Distinct beams always hold distinct folded prefixes: there is one beam at step 0, and the children of distinct
 * prefixes, or of one prefix under distinct fold symbols, are distinct.  So no merge across beams is needed, the k results
 * are k distinct folded strings, and with a trie's automaton k distinct words (out_tags).
 *
 * Approximation.  The hidden state follows the representative only: summed mass, Viterbi state - the usual prefix-merge
 * trade.  With all groups of one class (a case-sensitive pattern) the search IS the unmerged one, bit for bit.
 *
 * Path rows: expf(score_t - score_{t-1}) at the emitted (representative) symbol is the group's conditional mass, at most 1 up
 * to rounding; the word score exp(out_scores[:, 0]) (the model score when weighted) is the merged probability of the word.
 *
 * Needs what the unmerged search needs, and the group arrays; B == 0 returns GLASS_OK.  `workspace` >= the
 * merged_*_workspace_bytes(), which equal the unmerged searches'.  2 * max_len + 2 launches, ordinary grids with bounded
 * loops, no host synchronisation, no float atomics: results are bit-identical from run to run.                                */
int64_t glass_beam_search_merged_dfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len);
int glass_beam_search_merged_dfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                                 int C, int max_len, int eos, const int* next, const int* accept, const int* start,
                                 const int* fold, int N, int S, int F, const int* item_pattern, const int* group_start,
                                 const int* group_cls, int n_group_cls, int* out_symbols, float* out_scores, int* out_lengths,
                                 int* out_tags, float* out_path_probs, void* workspace, int64_t workspace_bytes,
                                 glass_stream_t stream);
int64_t glass_beam_search_merged_wdfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len);
int glass_beam_search_merged_wdfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                                  int C, int max_len, int eos, const glass_wdfa_transition* trans, const float* final_w,
                                  const float* start_w, const int* accept, const int* start, const int* fold, int N, int S,
                                  int F, const int* item_pattern, float weight_scale, const int* group_start,
                                  const int* group_cls, int n_group_cls, int* out_symbols, float* out_scores,
                                  float* out_model_scores, int* out_lengths, int* out_tags, float* out_path_probs,
                                  void* workspace, int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_MERGED_H */
