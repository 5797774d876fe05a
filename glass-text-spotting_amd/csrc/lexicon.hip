// glass_lexicon_match: the un-weighted branch of find_match_word (reference glass/evaluation/lexicon_utils.py:4-28).  The
// kernels and the description of the method are in lexicon_common.h, shared with lexicon_weighted.hip.
#include "lexicon_common.h"

extern "C" int64_t glass_lexicon_match_workspace_bytes(int Q) { return Q > 0 ? (int64_t)Q * 8 : 0; }

extern "C" int glass_lexicon_match(const uint8_t* q_sym, const int* q_len, const int* q_segment, int Q, const int* word_off,
                                   const int* word_len, const uint8_t* word_sym, const int* word_index, int L,
                                   const int* seg_off, int S, int max_segment_words, int* out_index, int* out_dist,
                                   void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(Q >= 0 && L >= 0 && S >= 0, "glass_lexicon_match: bad sizes Q=%d L=%d S=%d", Q, L, S);
  if (Q == 0) return GLASS_OK;
  GLASS_CHECK_ARG(q_sym && q_len && q_segment && out_index && out_dist && workspace, "glass_lexicon_match: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)q_sym & 3) == 0, "glass_lexicon_match: q_sym must be 4-byte aligned");
  GLASS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "glass_lexicon_match: workspace must be 8-byte aligned");
  GLASS_CHECK_ARG(workspace_bytes >= glass_lexicon_match_workspace_bytes(Q), "glass_lexicon_match: workspace of %lld bytes, needs %lld",
                  (long long)workspace_bytes, (long long)glass_lexicon_match_workspace_bytes(Q));
  const bool any_words = L > 0 && S > 0 && max_segment_words > 0;
  if (any_words) {
    GLASS_CHECK_ARG(word_off && word_len && word_sym && word_index && seg_off, "glass_lexicon_match: null pointer");
    GLASS_CHECK_ARG(((uintptr_t)word_sym & 15) == 0, "glass_lexicon_match: word_sym must be 16-byte aligned");
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* best = static_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(lexicon_init_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, best, Q);
  GLASS_CHECK_LAUNCH("glass_lexicon_match (init)");
  if (any_words) {
    const unsigned gx = (unsigned)cdiv(max_segment_words, LEX_CHUNK);
    const unsigned gy = (unsigned)min(Q, 65535);
    hipLaunchKernelGGL(lexicon_match_kernel, dim3(gx, gy), dim3(LEX_THREADS), 0, st, q_sym, q_len, q_segment, Q, word_off, word_len,
                       word_sym, word_index, L, seg_off, S, best);
    GLASS_CHECK_LAUNCH("glass_lexicon_match");
  }
  hipLaunchKernelGGL(lexicon_finalize_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, best, Q, out_index, out_dist);
  GLASS_CHECK_LAUNCH("glass_lexicon_match (finalize)");
  return GLASS_OK;
}
