/*
 * glass_hip_feature_dfa.h — entry points of libglass_hip.so (gfx950): pattern-constrained beam search.
 *
 * One header per feature (see glass_hip_feature_roimask.h): the earlier headers are closed, the binding parses every
 * include/glass_hip_feature_<feature>.h (glass_amd._lib.feature_signatures, FEATURE_EXPORTS).  Plain C, raw device pointers,
 * ints for sizes, 0 or a negative GLASS_E* code (glass_last_error() has the message), all work enqueued on the caller's stream,
 * nothing synchronises.  glass_abi_version() does not change.
 */
#ifndef GLASS_HIP_FEATURE_DFA_H
#define GLASS_HIP_FEATURE_DFA_H

#include "glass_hip.h" /* glass_decoder_weights, glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ beam search constrained by a finite automaton
 * glass_beam_search_lexicon (glass_hip_ext.h) with the trie generalised to any deterministic finite automaton (DFA) over
 * FOLD SYMBOLS: the hypotheses can only spell strings the automaton accepts (glass_amd.evaluation.pattern.DecodePattern
 * compiles a regex, a character set or a LexiconTrie into the tables).  Step arithmetic, selection rule, dead slots,
 * finalisation and outputs are those of glass_beam_search_lexicon, element for element; only the source of the mask differs:
 *   fold [C] ints: fold symbol 0..F-1 of every class, -1 for a class no string can contain; 1 <= F <= 256;
 *   next [N][F] ints, N >= 1 states: -1 = no transition, else the target state in bits 0..23 and
 *     min(dist[target], 127) in bits 24..30, dist[q] = the fewest symbols from q to an accepting state (any other negative
 *     entry counts as -1);
 *   accept [N] ints: -1 = not accepting, else a tag >= 0 that the result reports;
 *   start [S] ints, S >= 1: start state of every segment, -1 = a segment whose language is empty;
 *   item_pattern [B] ints: the segment of every item.
 * At step t (0-based, L = max_len) a beam in state q
 *   may emit class c != eos iff 0 <= fold[c] < F, e = next[q][fold[c]] >= 0 and t + 1 + (e >> 24) <= L - 1: the string can
 *     still be completed with its stop inside the L steps, so no live beam is a dead end;
 *   may emit `eos` iff accept[q] >= 0 and t >= 1 (the empty string is never emitted).
 * One 32-bit load per (beam, class) decides a candidate.  A selected finite candidate moves its slot to the target state
 * (`eos`: it stays, and the finalisation reports accept[q]).  Nothing read from the tables is used as an index unchecked: a
 * segment outside [0,S), a fold symbol outside [0,F), a start or target state outside [0,N) gives a dead slot.
 * Outputs as glass_beam_search_lexicon, with out_tags [B,k] = accept of the terminal state in the place of out_words (-1 for an
 * absent hypothesis).
 * Needs D == 256, 1 <= T <= 64, 1 <= C <= 256, 1 <= k <= 16, k <= C, 1 <= max_len <= 64, 1 <= N < 2^24, S >= 1,
 * 1 <= F <= 256; B == 0 returns GLASS_OK.  `workspace` (16-byte aligned) >= glass_beam_search_dfa_workspace_bytes(), which
 * equals glass_beam_search_lexicon_workspace_bytes().  2 * max_len + 2 launches, ordinary grids with bounded loops, no host
 * synchronisation, no float atomics: results are bit-identical from run to run.                                               */
int64_t glass_beam_search_dfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len);
int glass_beam_search_dfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D, int C,
                          int max_len, int eos, const int* next, const int* accept, const int* start, const int* fold, int N,
                          int S, int F, const int* item_pattern, int* out_symbols, float* out_scores, int* out_lengths,
                          int* out_tags, float* out_path_probs, void* workspace, int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_FEATURE_DFA_H */
