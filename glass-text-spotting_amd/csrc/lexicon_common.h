// The unit-cost lexicon matcher shared by csrc/lexicon.hip (glass_lexicon_match) and csrc/lexicon_weighted.hip (stage 1 and
// the candidate filter of glass_lexicon_match_weighted).  Internal linkage: each file that includes it has its own copy.
//
// Lexicon matching for lexicon-constrained text evaluation: for each recognised word (query), the closest word of its
// lexicon segment by unit-cost Levenshtein distance, first strict minimum in file order (reference
// glass/evaluation/lexicon_utils.py:4-28, the un-weighted branch of find_match_word).
//
// Distance: bit-parallel (Myers 1999 / Hyyro 2003) with the QUERY as the pattern (m <= 64 symbols in one 64-bit word)
// and the lexicon word as the streamed text (any length).  Global edit distance: the top DP row is 0..n, so the
// horizontal-positive vector shifts in a 1, and the score starts at m.  Bits above m - 1 hold garbage that never reaches
// the low m bits (additions and left shifts only carry upwards).
//
// Layout: one workgroup takes one query and chunks of LEX_CHUNK words of that query's segment (grid-stride in x), each
// lane one word at a time.  The query's match masks Peq live in LDS, 256 entries so that the sentinel symbol of
// non-ASCII lexicon characters (>= 128, never in a query) reads an empty mask without a branch.  Lanes keep the
// packed key (dist << 32) | original index of their best word; a wave reduction, an LDS step over the 4 waves, and
// one vector 64-bit atomicMin per workgroup combine them.  The minimum of the packed keys is the smallest
// (distance, original index), so the result does not depend on the order the workgroups run in.
#pragma once
#include "common.h"

namespace {

constexpr int LEX_THREADS = 256;
constexpr int LEX_WAVES = LEX_THREADS / 64;
constexpr int LEX_WORDS_PER_LANE = 4;
constexpr int LEX_CHUNK = LEX_THREADS * LEX_WORDS_PER_LANE;
constexpr int LEX_DIST_NONE = 100;                                       // the reference's dist_min start value
constexpr unsigned long long LEX_KEY_NONE = ((unsigned long long)LEX_DIST_NONE << 32) | 0xffffffffull;

__global__ void lexicon_init_kernel(unsigned long long* best, int Q) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < Q) best[q] = LEX_KEY_NONE;
}

__global__ void lexicon_finalize_kernel(const unsigned long long* best, int Q, int* out_index, int* out_dist) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const unsigned long long k = best[q];
  const int d = (int)(k >> 32);
  const bool hit = d < LEX_DIST_NONE;
  out_index[q] = hit ? (int)(unsigned)(k & 0xffffffffull) : -1;
  out_dist[q] = hit ? d : LEX_DIST_NONE;
}

// edit distance between the pattern held in `peq` (m symbols, 1 <= m <= 64) and the n symbols at `sym` (16-byte aligned)
__device__ __forceinline__ int myers_distance(const unsigned long long* peq, int m, const unsigned char* sym, int n) {
  const unsigned long long hb = 1ull << (m - 1);
  unsigned long long pv = ~0ull, mv = 0ull;
  int score = m;
  for (int base = 0; base < n; base += 16) {
    const uint4 piece = *reinterpret_cast<const uint4*>(sym + base);
    const unsigned w4[4] = {piece.x, piece.y, piece.z, piece.w};
    const int cnt = min(16, n - base);
    // all 16 masks first (a padding byte reads some entry of the table: harmless), so the LDS latency is paid once per piece
    unsigned long long eqs[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) eqs[t] = peq[(w4[t >> 2] >> (8 * (t & 3))) & 0xffu];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (t < cnt) {
        const unsigned long long eq = eqs[t];
        const unsigned long long xv = eq | mv;
        const unsigned long long xh = (((eq & pv) + pv) ^ pv) | eq;
        unsigned long long ph = mv | ~(xh | pv);
        unsigned long long mh = pv & xh;
        score += (ph & hb) ? 1 : ((mh & hb) ? -1 : 0);
        ph = (ph << 1) | 1ull;                                           // global distance: row 0 is 0..n
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
      }
    }
  }
  return score;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(LEX_THREADS) void lexicon_match_kernel(
    const unsigned char* __restrict__ q_sym, const int* __restrict__ q_len, const int* __restrict__ q_segment, int Q,
    const int* __restrict__ word_off, const int* __restrict__ word_len, const unsigned char* __restrict__ word_sym,
    const int* __restrict__ word_index, int L, const int* __restrict__ seg_off, int S, unsigned long long* best_key) {
  __shared__ unsigned long long peq[256];
  __shared__ unsigned long long wave_best[LEX_WAVES];
  __shared__ unsigned qbuf[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    const int s = q_segment[q];
    int b = 0, e = 0;
    if (s >= 0 && s < S) {
      b = min(max(seg_off[s], 0), L);
      e = min(max(seg_off[s + 1], b), L);
    }
    if (b + (long)blockIdx.x * LEX_CHUNK >= e) continue;                 // uniform over the workgroup
    const int m = min(max(q_len[q], 0), 64);
    __syncthreads();                                                     // the previous query's readers are done
    if (tid < 16) qbuf[tid] = reinterpret_cast<const unsigned*>(q_sym + (size_t)q * 64)[tid];
    __syncthreads();
    {
      const unsigned char* qs = reinterpret_cast<const unsigned char*>(qbuf);
      unsigned long long eq = 0ull;
      if (tid < 128)
        for (int j = 0; j < m; ++j) eq |= (qs[j] == (unsigned)tid) ? (1ull << j) : 0ull;
      peq[tid] = eq;
    }
    __syncthreads();
    unsigned long long best = LEX_KEY_NONE;
    int best_d = LEX_DIST_NONE;
    for (long c0 = b + (long)blockIdx.x * LEX_CHUNK; c0 < e; c0 += (long)gridDim.x * LEX_CHUNK) {
      for (int k = 0; k < LEX_WORDS_PER_LANE; ++k) {
        const long i = c0 + k * LEX_THREADS + tid;
        if (i >= e) break;
        const int n = word_len[i];
        // dist >= |m - n|: a word that cannot reach the lane's best (ties included) or the acceptance bound is skipped
        if (abs(m - n) > min(best_d, LEX_DIST_NONE - 1)) continue;
        const int d = m == 0 ? n : myers_distance(peq, m, word_sym + word_off[i], n);
        if (d < LEX_DIST_NONE) {
          const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)word_index[i];
          if (key < best) {
            best = key;
            best_d = d;
          }
        }
      }
    }
    best = wave_min_u64(best);
    if (lane == 0) wave_best[wid] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned long long k = wave_best[0];
      for (int w = 1; w < LEX_WAVES; ++w) k = wave_best[w] < k ? wave_best[w] : k;
      if (k < LEX_KEY_NONE) atomicMin(best_key + q, k);
    }
  }
}

}  // namespace
