/*
 * glass_hip_ext.h — additive entry points of libglass_hip.so (gfx950) that came after the set of glass_hip.h was closed.
 *
 * glass_hip.h stays as it is (its set of prototypes is pinned by the host tests); an entry point added to the library is
 * declared HERE.  Same conventions as glass_hip.h: plain C, raw device pointers, ints for sizes, every function returns 0 or
 * a negative GLASS_E* code (glass_last_error() has the message), all work is enqueued on the caller's stream, nothing
 * synchronises unless stated.  The additions do not change glass_abi_version(): a binding finds them by symbol.
 */
#ifndef GLASS_HIP_EXT_H
#define GLASS_HIP_EXT_H

#include "glass_hip.h" /* glass_decoder_weights, glass_stream_t, GLASS_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ lexicon-constrained beam search (evaluation)
 * glass_beam_search whose hypotheses can only spell words of a lexicon: the decoder returns the k most likely lexicon words
 * under the model, with their log-likelihoods (the "constrained decoding" protocol of the IC15 strong / weak / generic and
 * Total-Text lexicons).  The reference has no such function (AttentionRecognitionHead.beam_search, prediction_aster.py:101-222,
 * is unconstrained); the step arithmetic is glass_beam_search's, element for element.  Inputs, packing and limits as
 * glass_beam_search, plus the lexicon as a trie over FOLD SYMBOLS (glass_amd.evaluation.lexicon.LexiconTrie builds it):
 *   fold [C] ints: fold symbol 0..F-1 of every class (a character and its other case share one), -1 for a class no word
 *     can contain ([GO], the stop, [UNK], ...); 1 <= F <= 256, MW = (F + 31) / 32 mask words per node;
 *   N >= 1 nodes in breadth-first order, the children of a node contiguous and ordered by fold symbol:
 *     child_mask [N][MW] 32-bit words (bit f set: the node has a child for fold symbol f), child_base [N] ints,
 *     child(node, f) = child_base[node] + popcount(mask bits below f);
 *     node_word [N] ints: -1, or the index of the first lexicon word that ends at the node;
 *   seg_root [S] ints, S >= 1: root node of every segment (one per image of a per-image lexicon), -1 = an empty segment;
 *   item_segment [B] ints: the segment of every item.
 * Per step, candidate (beam r, class c) keeps its score only if c != eos, 0 <= fold[c] < F and bit fold[c] of
 * child_mask[node_r] is set, or c == eos and node_word[node_r] >= 0 (for c == eos only this second rule counts); every other
 * candidate, every candidate of a dead beam and everything of an item whose segment is outside [0,S) or empty is -inf.
 * Selection as in glass_beam_search (score descending, then flat index beam*C + class; -inf last in index order).  A selected
 * -inf candidate leaves a dead slot: no node, never finite again, its recorded symbol still a valid class.  A selected finite
 * candidate moves its slot to the child node (`eos`: it records the terminal node, and the beam is frozen at -inf as in
 * glass_beam_search).  Nothing read from the arrays is used as an index unchecked: a fold symbol outside [0,F), a root or
 * a child outside [0,N) gives a dead slot.
 * Finalisation, one wavefront per item (NOT the reference's back-tracking): the completed entries are the table entries
 * (t, slot) whose symbol is `eos` and whose score is finite; the result is the k best of them by score descending, then t,
 * then slot ascending, each walked back through the predecessor table:
 *   out_symbols [B,k,max_len] ints (`eos` from the length on), out_scores [B,k], out_lengths [B,k] = t + 1,
 *   out_words [B,k] = node_word of the terminal node (two case variants of one word are two hypotheses with one word index);
 *   with fewer than k completions the remaining hypotheses have score -inf, length 0, word -1 and all-`eos` symbols;
 *   out_path_probs [B,max_len,C] or null: as in glass_beam_search - row t < length of the best hypothesis is zero except
 *   exp(score_t - score_{t-1}) at symbols[t]; every other row, and every row of a -inf best, is zero.
 * Needs D == 256, 1 <= T <= 64, 1 <= C <= 256, 1 <= k <= 16, k <= C, 1 <= max_len <= 64, N >= 1, S >= 1, 1 <= F <= 256;
 * B == 0 returns GLASS_OK.  `workspace` (16-byte aligned) >= glass_beam_search_lexicon_workspace_bytes().  2 * max_len + 2
 * launches, ordinary grids with bounded loops, no host synchronisation, no float atomics: results are bit-identical from run
 * to run.  The mask costs a thread at most k 32-bit loads per step.                                                        */
int64_t glass_beam_search_lexicon_workspace_bytes(int B, int k, int T, int D, int C, int max_len);
int glass_beam_search_lexicon(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                              int C, int max_len, int eos, const uint32_t* child_mask, const int* child_base,
                              const int* node_word, const int* seg_root, const int* fold, int N, int S, int F,
                              const int* item_segment, int* out_symbols, float* out_scores, int* out_lengths, int* out_words,
                              float* out_path_probs, void* workspace, int64_t workspace_bytes, glass_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_HIP_EXT_H */
