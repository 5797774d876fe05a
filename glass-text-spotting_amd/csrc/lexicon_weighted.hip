// glass_lexicon_match_weighted: the weighted branch of find_match_word (reference glass/evaluation/lexicon_utils.py:26-48 and
// weighted_edit_distance :136-182, MaskTextSpotterV3's LEXICON_WEIGHTED): candidates are the words within dist_min_pre + 2
// unit edits of the query, and the winner is the first candidate in file order with the strictly smallest weighted edit
// distance below 100.  The weighted distance is a float64 DP whose costs depend on the query position (deletion,
// insertion) and on (query position, class of the word symbol) (substitution); the host builds those tables per query
// (glass_amd/evaluation/lexicon.py) and the kernel only adds and takes minima, each cell with the three additions of the
// reference in float64, so the result has the reference's bits.  Contraction is off for the file; there is nothing to
// contract, and it must stay that way.
//
// Stage 1: the un-weighted kernel of lexicon_common.h gives every query's smallest unit distance (dist_min_pre, 100 if no
//   word is closer).
// Stage 2 (lexw_kernel): one workgroup takes one query and one slice of its segment.  It walks the slice LEX_CHUNK words at a
//   time, each lane up to 4 words: length filter |m - n| <= dist_min_pre + 2, bit-parallel unit distance, and the survivors'
//   positions are compacted into an LDS list (ballot + popcount, wave bases through LDS: a fixed order).  Whenever 256 are
//   pending, and once at the end of the slice, the DP runs one candidate per lane, so its lanes are full however few words
//   of a chunk survive.  The DP row lives in registers (the j loop is unrolled to the bucket M >= the launch's longest
//   query); del / ins / rep tables of the query are in LDS (rep stays in global memory when the launch's largest table
//   does not fit 64 KiB).  Each lane keeps the smallest (distance bits, original index); wave shuffle, LDS over the 4
//   waves, one partial per (query, slice).
// Finalize: one thread per query takes the minimum over the slices in slice order.  No floating-point atomics; the result
//   does not depend on the order workgroups run in.
//
// A candidate symbol without a class (cls >= A) sets bit 0 of the query's status word (char_encode's KeyError upstream);
// a query whose length or table offset is out of range sets bit 1 and matches nothing.
#include "lexicon_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LEXW_BATCH = LEX_THREADS;                                  // candidates per DP round: one per lane
constexpr int LEXW_LIST = LEX_CHUNK + LEXW_BATCH;                        // pending candidates: < BATCH left over + one chunk
constexpr int LEXW_TARGET_GROUPS = 4096;                                 // slices are cut until a launch has about this many workgroups
constexpr double LEXW_DIST_NONE = 100.0;
constexpr unsigned long long LEXW_BITS_NONE = ~0ull;
// LDS carve (bytes; every offset a multiple of 16)
constexpr int LEXW_OFF_PEQ = 0;                                          // 256 x u64
constexpr int LEXW_OFF_LIST = LEXW_OFF_PEQ + 256 * 8;                    // LEXW_LIST x i32
constexpr int LEXW_OFF_CLS = LEXW_OFF_LIST + LEXW_LIST * 4;              // 256 x u8
constexpr int LEXW_OFF_QBUF = LEXW_OFF_CLS + 256;                        // 64 x u8
constexpr int LEXW_OFF_WCNT = LEXW_OFF_QBUF + 64;                        // 4 x i32
constexpr int LEXW_OFF_WIDX = LEXW_OFF_WCNT + 16;                        // 4 x u32
constexpr int LEXW_OFF_WBITS = LEXW_OFF_WIDX + 16;                       // 4 x u64
constexpr int LEXW_OFF_COST = LEXW_OFF_WBITS + 32;                       // del[m], ins[m] (, rep[m][A]) as doubles
constexpr int LEXW_LDS_MAX = 64 * 1024;
static_assert(LEXW_OFF_COST % 16 == 0 && LEXW_OFF_LIST % 16 == 0 && LEXW_OFF_CLS % 16 == 0, "LDS carve alignment");

inline int lexw_chunks(int max_segment_words) { return max_segment_words > 0 ? cdiv(max_segment_words, LEX_CHUNK) : 0; }
// slices per query: 1 when the queries alone fill the device, up to one per chunk for a handful of queries
inline int lexw_slices(int Q, int max_segment_words) {
  const int chunks = lexw_chunks(max_segment_words);
  if (Q <= 0 || chunks <= 0) return 0;
  return max(1, min(chunks, cdiv(LEXW_TARGET_GROUPS, Q)));
}

__global__ void lexw_init_kernel(unsigned long long* best, int* out_status, int Q) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < Q) {
    best[q] = LEX_KEY_NONE;
    out_status[q] = 0;
  }
}

__device__ __forceinline__ bool lexw_less(unsigned long long ab, unsigned ai, unsigned long long bb, unsigned bi) {
  return ab < bb || (ab == bb && ai < bi);
}

__global__ void lexw_finalize_kernel(const unsigned long long* __restrict__ pbits, const unsigned* __restrict__ pidx, int slices,
                                     int Q, int* out_index, double* out_dist) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  unsigned long long bits = LEXW_BITS_NONE;
  unsigned idx = 0xffffffffu;
  for (int x = 0; x < slices; ++x) {
    const unsigned long long b = pbits[(size_t)q * slices + x];
    const unsigned i = pidx[(size_t)q * slices + x];
    if (lexw_less(b, i, bits, idx)) {
      bits = b;
      idx = i;
    }
  }
  const bool hit = bits != LEXW_BITS_NONE;
  out_index[q] = hit ? (int)idx : -1;
  out_dist[q] = hit ? __longlong_as_double((long long)bits) : LEXW_DIST_NONE;
}

struct LexwArgs {
  const unsigned char* q_sym;
  const int* q_len;
  const int* q_segment;
  int Q;
  const double* cost;
  long long cost_doubles;
  const long long* q_cost_off;
  const unsigned char* sym_class;
  int A;
  int max_m;
  const int* word_off;
  const int* word_len;
  const unsigned char* word_sym;
  const int* word_index;
  int L;
  const int* seg_off;
  int S;
  long slice_words;
  int slices;
  const unsigned long long* best_key;
  unsigned long long* pbits;
  unsigned* pidx;
  int* out_status;
};

template <int M, bool REP_LDS>
__global__ __launch_bounds__(LEX_THREADS) void lexw_kernel(const LexwArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* peq = reinterpret_cast<unsigned long long*>(smem + LEXW_OFF_PEQ);
  int* list = reinterpret_cast<int*>(smem + LEXW_OFF_LIST);
  unsigned char* cls = smem + LEXW_OFF_CLS;
  unsigned* qbuf = reinterpret_cast<unsigned*>(smem + LEXW_OFF_QBUF);
  int* wave_cnt = reinterpret_cast<int*>(smem + LEXW_OFF_WCNT);
  unsigned* wave_idx = reinterpret_cast<unsigned*>(smem + LEXW_OFF_WIDX);
  unsigned long long* wave_bits = reinterpret_cast<unsigned long long*>(smem + LEXW_OFF_WBITS);
  double* cost_s = reinterpret_cast<double*>(smem + LEXW_OFF_COST);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int A = p.A;
  cls[tid] = p.sym_class[tid];                                           // LEX_THREADS == 256 entries; the loop below syncs before use
  for (int q = blockIdx.y; q < p.Q; q += gridDim.y) {
    const size_t part = (size_t)q * p.slices + blockIdx.x;
    const int s = p.q_segment[q];
    int b = 0, e = 0;
    if (s >= 0 && s < p.S) {
      b = min(max(p.seg_off[s], 0), p.L);
      e = min(max(p.seg_off[s + 1], b), p.L);
    }
    const long lo = b + (long)blockIdx.x * p.slice_words;
    const long hi = min((long)e, lo + p.slice_words);
    const int m = p.q_len[q];
    const long long off = p.q_cost_off[q];
    const bool bad_query = m < 0 || m > p.max_m || m > M || off < 0 || off + (long long)m * (A + 2) > p.cost_doubles;
    if (lo >= hi || bad_query) {                                         // uniform over the workgroup
      if (tid == 0) {
        p.pbits[part] = LEXW_BITS_NONE;
        p.pidx[part] = 0xffffffffu;
        if (bad_query) atomicOr(p.out_status + q, 2);
      }
      continue;
    }
    __syncthreads();                                                     // the previous query's readers are done
    if (tid < 16) qbuf[tid] = reinterpret_cast<const unsigned*>(p.q_sym + (size_t)q * 64)[tid];
    for (int k = tid; k < (REP_LDS ? m * (A + 2) : 2 * m); k += LEX_THREADS) cost_s[k] = p.cost[off + k];
    __syncthreads();
    const unsigned char* qs = reinterpret_cast<const unsigned char*>(qbuf);
    {
      unsigned long long eq = 0ull;
      if (tid < 128)
        for (int j = 0; j < m; ++j) eq |= (qs[j] == (unsigned)tid) ? (1ull << j) : 0ull;
      peq[tid] = eq;
    }
    __syncthreads();
    const double* del_c = cost_s;
    const double* ins_c = cost_s + m;
    const int bound = min((int)(p.best_key[q] >> 32), LEX_DIST_NONE) + 2;  // dist_min_pre + 2
    unsigned long long best_bits = LEXW_BITS_NONE;
    unsigned best_idx = 0xffffffffu;
    bool no_class = false;

    // the DP of `cnt` (1..LEXW_BATCH) pending candidates at list[from ..], one per lane
    auto dp_round = [&](int from, int cnt) {
      const int ci = tid < cnt ? list[from + tid] : -1;
      __syncthreads();                                                   // the list may be appended to from here on
      if (ci < 0) return;
      const int n = max(p.word_len[ci], 0);
      const unsigned char* sym = p.word_sym + p.word_off[ci];
      double r[M + 1];
#pragma unroll
      for (int j = 0; j <= M; ++j) r[j] = (double)j;                     // dp[0][j] = j
      for (int base = 0; base < n; base += 16) {
        const uint4 piece = *reinterpret_cast<const uint4*>(sym + base);
        const int cnt16 = min(16, n - base);
#pragma unroll 1
        for (int t = 0; t < cnt16; ++t) {
          const unsigned w4 = (t & 8) ? ((t & 4) ? piece.w : piece.z) : ((t & 4) ? piece.y : piece.x);
          const unsigned ws = (w4 >> (8 * (t & 3))) & 0xffu;
          unsigned a = cls[ws];
          if (a >= (unsigned)A) {
            no_class = true;
            a = 0;
          }
          double diag = r[0];
          r[0] = diag + 1.0;                                             // dp[i][0] = i
#pragma unroll
          for (int j = 1; j <= M; ++j) {
            if (j <= m) {                                                // uniform
              const double up = r[j];
              double rep = 0.0;
              if (qs[j - 1] != ws)
                rep = REP_LDS ? cost_s[2 * m + (j - 1) * A + a] : p.cost[off + 2 * m + (long long)(j - 1) * A + a];
              const double v = fmin(fmin(up + ins_c[j - 1], r[j - 1] + del_c[j - 1]), diag + rep);
              diag = up;
              r[j] = v;
            }
          }
        }
      }
      double dist = r[0];
#pragma unroll
      for (int j = 1; j <= M; ++j)
        if (j == m) dist = r[j];
      if (dist < LEXW_DIST_NONE) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(dist);
        const unsigned idx = (unsigned)p.word_index[ci];
        if (lexw_less(bits, idx, best_bits, best_idx)) {
          best_bits = bits;
          best_idx = idx;
        }
      }
    };

    int count = 0;                                                       // pending candidates; the same value in every thread
    for (long c0 = lo; c0 < hi; c0 += LEX_CHUNK) {
      unsigned long long bal[LEX_WORDS_PER_LANE];
      unsigned mine = 0;
#pragma unroll
      for (int k = 0; k < LEX_WORDS_PER_LANE; ++k) {
        const long i = c0 + k * LEX_THREADS + tid;
        bool ok = false;
        if (i < hi) {
          const int n = p.word_len[i];
          if (n >= 0 && abs(m - n) <= bound) {                           // dist >= |m - n|
            const int d = m == 0 ? n : myers_distance(peq, m, p.word_sym + p.word_off[i], n);
            ok = d <= bound;
          }
        }
        bal[k] = __ballot(ok);
        mine |= ok ? (1u << k) : 0u;
      }
      int wave_total = 0;
#pragma unroll
      for (int k = 0; k < LEX_WORDS_PER_LANE; ++k) wave_total += __popcll(bal[k]);
      if (lane == 0) wave_cnt[wid] = wave_total;
      __syncthreads();
      int pos = count, total = 0;
#pragma unroll
      for (int w = 0; w < LEX_WAVES; ++w) {
        const int c = wave_cnt[w];
        pos += w < wid ? c : 0;
        total += c;
      }
      const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
      for (int k = 0; k < LEX_WORDS_PER_LANE; ++k) {
        if (mine & (1u << k)) list[pos + __popcll(bal[k] & below)] = (int)(c0 + k * LEX_THREADS + tid);
        pos += __popcll(bal[k]);
      }
      count += total;                                                    // <= LEXW_BATCH - 1 + LEX_CHUNK < LEXW_LIST
      __syncthreads();
      while (count >= LEXW_BATCH) {
        count -= LEXW_BATCH;
        dp_round(count, LEXW_BATCH);
      }
    }
    if (count > 0) dp_round(0, count);

    if (no_class && m > 0) atomicOr(p.out_status + q, 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ob = __shfl_xor(best_bits, o);
      const unsigned oi = __shfl_xor(best_idx, o);
      if (lexw_less(ob, oi, best_bits, best_idx)) {
        best_bits = ob;
        best_idx = oi;
      }
    }
    if (lane == 0) {
      wave_bits[wid] = best_bits;
      wave_idx[wid] = best_idx;
    }
    __syncthreads();
    if (tid == 0) {
      unsigned long long kb = wave_bits[0];
      unsigned ki = wave_idx[0];
      for (int w = 1; w < LEX_WAVES; ++w)
        if (lexw_less(wave_bits[w], wave_idx[w], kb, ki)) {
          kb = wave_bits[w];
          ki = wave_idx[w];
        }
      p.pbits[part] = kb;
      p.pidx[part] = ki;
    }
  }
}

template <int M>
void lexw_launch(const LexwArgs& a, dim3 grid, int lds_rep, int lds_norep, hipStream_t st) {
  if (lds_rep <= LEXW_LDS_MAX)
    hipLaunchKernelGGL((lexw_kernel<M, true>), grid, dim3(LEX_THREADS), lds_rep, st, a);
  else
    hipLaunchKernelGGL((lexw_kernel<M, false>), grid, dim3(LEX_THREADS), lds_norep, st, a);
}

}  // namespace

extern "C" int64_t glass_lexicon_match_weighted_workspace_bytes(int Q, int max_segment_words) {
  if (Q <= 0) return 0;
  const int64_t parts = (int64_t)Q * lexw_slices(Q, max_segment_words);
  return (int64_t)Q * 8 + parts * 8 + (parts * 4 + 7) / 8 * 8;
}

extern "C" int glass_lexicon_match_weighted(const uint8_t* q_sym, const int* q_len, const int* q_segment, int Q, const double* cost,
                                            int64_t cost_doubles, const int64_t* q_cost_off, const uint8_t* sym_class, int A,
                                            int max_query_len, const int* word_off, const int* word_len, const uint8_t* word_sym,
                                            const int* word_index, int L, const int* seg_off, int S, int max_segment_words,
                                            int* out_index, double* out_dist, int* out_status, void* workspace,
                                            int64_t workspace_bytes, glass_stream_t stream) {
  const char* me = "glass_lexicon_match_weighted";
  GLASS_CHECK_ARG(Q >= 0 && L >= 0 && S >= 0, "%s: bad sizes Q=%d L=%d S=%d", me, Q, L, S);
  if (Q == 0) return GLASS_OK;
  GLASS_CHECK_ARG(A >= 1 && A <= 255, "%s: A=%d classes (1..255)", me, A);
  GLASS_CHECK_ARG(max_query_len >= 0 && max_query_len <= 64, "%s: max_query_len=%d (0..64)", me, max_query_len);
  GLASS_CHECK_ARG(cost_doubles >= 0, "%s: cost_doubles=%lld", me, (long long)cost_doubles);
  GLASS_CHECK_ARG(q_sym && q_len && q_segment && q_cost_off && sym_class && out_index && out_dist && out_status && workspace,
                  "%s: null pointer", me);
  GLASS_CHECK_ARG(cost || cost_doubles == 0, "%s: null cost table", me);
  GLASS_CHECK_ARG(((uintptr_t)q_sym & 3) == 0, "%s: q_sym must be 4-byte aligned", me);
  GLASS_CHECK_ARG(((uintptr_t)cost & 7) == 0 && ((uintptr_t)q_cost_off & 7) == 0 && ((uintptr_t)out_dist & 7) == 0,
                  "%s: cost, q_cost_off and out_dist must be 8-byte aligned", me);
  GLASS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", me);
  const int64_t need = glass_lexicon_match_weighted_workspace_bytes(Q, max_segment_words);
  GLASS_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %lld bytes, needs %lld", me, (long long)workspace_bytes, (long long)need);
  const bool any_words = L > 0 && S > 0 && max_segment_words > 0;
  if (any_words) {
    GLASS_CHECK_ARG(word_off && word_len && word_sym && word_index && seg_off, "%s: null pointer", me);
    GLASS_CHECK_ARG(((uintptr_t)word_sym & 15) == 0, "%s: word_sym must be 16-byte aligned", me);
  }
  hipStream_t st = (hipStream_t)stream;
  const int slices = any_words ? lexw_slices(Q, max_segment_words) : 0;
  unsigned long long* best = static_cast<unsigned long long*>(workspace);
  unsigned long long* pbits = best + Q;
  unsigned* pidx = reinterpret_cast<unsigned*>(pbits + (size_t)Q * lexw_slices(Q, max_segment_words));
  hipLaunchKernelGGL(lexw_init_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, best, out_status, Q);
  GLASS_CHECK_LAUNCH("glass_lexicon_match_weighted (init)");
  if (any_words) {
    const unsigned gy = (unsigned)min(Q, 65535);
    hipLaunchKernelGGL(lexicon_match_kernel, dim3((unsigned)lexw_chunks(max_segment_words), gy), dim3(LEX_THREADS), 0, st, q_sym,
                       q_len, q_segment, Q, word_off, word_len, word_sym, word_index, L, seg_off, S, best);
    GLASS_CHECK_LAUNCH("glass_lexicon_match_weighted (stage 1)");
    LexwArgs a;
    a.q_sym = q_sym; a.q_len = q_len; a.q_segment = q_segment; a.Q = Q;
    a.cost = cost; a.cost_doubles = cost_doubles; a.q_cost_off = reinterpret_cast<const long long*>(q_cost_off);
    a.sym_class = sym_class; a.A = A; a.max_m = max_query_len;
    a.word_off = word_off; a.word_len = word_len; a.word_sym = word_sym; a.word_index = word_index; a.L = L;
    a.seg_off = seg_off; a.S = S;
    a.slice_words = (long)cdiv(lexw_chunks(max_segment_words), slices) * LEX_CHUNK;
    a.slices = slices;
    a.best_key = best; a.pbits = pbits; a.pidx = pidx; a.out_status = out_status;
    const int lds_rep = LEXW_OFF_COST + max_query_len * (A + 2) * 8, lds_norep = LEXW_OFF_COST + max_query_len * 2 * 8;
    const dim3 grid((unsigned)slices, gy);
    if (max_query_len <= 8) lexw_launch<8>(a, grid, lds_rep, lds_norep, st);
    else if (max_query_len <= 16) lexw_launch<16>(a, grid, lds_rep, lds_norep, st);
    else if (max_query_len <= 32) lexw_launch<32>(a, grid, lds_rep, lds_norep, st);
    else lexw_launch<64>(a, grid, lds_rep, lds_norep, st);
    GLASS_CHECK_LAUNCH("glass_lexicon_match_weighted (stage 2)");
  }
  hipLaunchKernelGGL(lexw_finalize_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, st, pbits, pidx, slices, Q, out_index, out_dist);
  GLASS_CHECK_LAUNCH("glass_lexicon_match_weighted (finalize)");
  return GLASS_OK;
}
