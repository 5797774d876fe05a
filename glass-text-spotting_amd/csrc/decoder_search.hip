// Searches over the attention-GRU decoder of decoder.hip, each behind one ABI call with no host synchronisation: beam search,
// forced decoding (the symbols given) and the constrained beam searches (a lexicon trie, any DFA, or a weighted DFA; the two
// automaton searches also fold-merged).  Per step they run the decoder's GRU launch (dec_gru_step) on all rows and one step
// kernel, one workgroup per item, composed of the rows_* pieces of decoder_common.h.  The six beam searches share one
// workspace layout (beam_layout) and one host driver (run_beam_search); forced decoding keeps its own loop.
#include <type_traits>
#include "decoder_common.h"
#include "glass_hip_ext.h"
#include "glass_hip_feature_chars.h"
#include "glass_hip_feature_dfa.h"
#include "glass_hip_feature_merged.h"
#include "glass_hip_feature_wdfa.h"

// ================================================================== beam search (AttentionRecognitionHead.beam_search)
// The whole search of reference prediction_aster.py:101-222 behind one ABI call: per step dec_gru_kernel on the B*k state rows
// and beam_step_kernel (one workgroup per batch item), then one beam_backtrack_kernel (one wavefront per item).  No host
// synchronisation, no read-back; x / xproj stay [B,T,D]: an item's rows are read once per step and serve its k beams.
//   workspace: hsel [B*k,D] (states gathered by predecessor = the GRU's h_prev) | hraw [B*k,D] (the GRU's output) |
//              inp [B*k,2D] | score, predecessor and symbol tables [B,L,k] each (predecessors are beam slots 0..k-1)
// Selection rule (torch.topk leaves ties open): candidates ordered by score descending, then by flat index beam*C + class
// ascending; -inf candidates last, in index order.
struct BeamParams {
  float* sc; int* pr; int* sy;      // decision tables [B][L][k]
  float* hsel;                      // [B*k][D]
  int k, L, eos;
};

// ---- host side, shared by all the searches
// f(std::integral_constant<int, KB>) with KB = k rounded up to 1, 2, 4, 8 or 16, the row blocking of the step kernels
template <class F>
static void with_row_block(int k, F f) {
  if (k == 1) f(std::integral_constant<int, 1>{});
  else if (k == 2) f(std::integral_constant<int, 2>{});
  else if (k <= 4) f(std::integral_constant<int, 4>{});
  else if (k <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

// the limits of a search with k rows per item: `beams` = the rows are k beams, which must also fit the classes; else they are
// n given sequences
static int search_limits(const char* fn, bool beams, int B, int k, int T, int D, int C, int max_len) {
  const char* kn = beams ? "k" : "n";
  GLASS_CHECK_ARG(D == DEC_D && T > 0 && T <= DEC_TMAX && C > 0 && C <= DEC_CMAX && k >= 1 && k <= BEAM_KMAX && (!beams || k <= C) &&
                      max_len >= 1 && max_len <= BEAM_LMAX && B >= 0,
                  "%s: needs D=256, 1<=T<=64, 1<=C<=256, 1<=%s<=16, %s1<=max_len<=64, B>=0 (got B=%d %s=%d T=%d D=%d C=%d max_len=%d)",
                  fn, kn, beams ? "k<=C, " : "", B, kn, k, T, D, C, max_len);
  return GLASS_OK;
}

// the workspace of the six beam searches as byte offsets and its size: hsel | hraw | inp (2x) | sc | pr | sy | nd | wa | fu, a
// state block B*k*D floats, a table B*L*k floats (the int tables are as large).  nd (the constrained searches' node table),
// wa and fu (the weighted search's weight sums and fused scores) take room only where `has` names them.  Every
// *_workspace_bytes function and beam_carve read it; a size that is not positive gives the empty layout.
struct BeamTables { bool nd, wa, fu; };
constexpr BeamTables BEAM_PLAIN = {false, false, false}, BEAM_NODES = {true, false, false}, BEAM_WEIGHTED = {true, true, true};
struct BeamLayout { size_t hsel, hraw, inp, sc, pr, sy, nd, wa, fu, total; };
static BeamLayout beam_layout(int B, int k, int D, int L, BeamTables has) {
  if (B <= 0 || k <= 0 || D <= 0 || L <= 0) return {};
  const size_t state = (size_t)B * k * D * sizeof(float), table = (size_t)B * L * k * sizeof(float);
  BeamLayout o;
  o.hsel = 0; o.hraw = o.hsel + state; o.inp = o.hraw + state; o.sc = o.inp + 2 * state; o.pr = o.sc + table; o.sy = o.pr + table;
  o.nd = o.sy + table; o.wa = o.nd + (has.nd ? table : 0); o.fu = o.wa + (has.wa ? table : 0);
  o.total = o.fu + (has.fu ? table : 0);
  return o;
}
// p.h0 = hsel (the GRU's h_prev), p.h1 = hraw (its output), p.inp and the tables of bp point into `workspace`; the tables a
// search does not have stay null
struct BeamCarved { BeamParams bp; int* nd; float* wa; float* fu; };
static BeamCarved beam_carve(void* workspace, const BeamLayout& o, BeamTables has, int k, int L, int eos, DecParams& p) {
  char* ws = static_cast<char*>(workspace);
  p.h0 = reinterpret_cast<float*>(ws + o.hsel); p.h1 = reinterpret_cast<float*>(ws + o.hraw); p.inp = reinterpret_cast<float*>(ws + o.inp);
  BeamCarved c = {};
  c.bp.sc = reinterpret_cast<float*>(ws + o.sc); c.bp.pr = reinterpret_cast<int*>(ws + o.pr); c.bp.sy = reinterpret_cast<int*>(ws + o.sy);
  c.bp.hsel = p.h0; c.bp.k = k; c.bp.L = L; c.bp.eos = eos;
  if (has.nd) c.nd = reinterpret_cast<int*>(ws + o.nd);
  if (has.wa) c.wa = reinterpret_cast<float*>(ws + o.wa);
  if (has.fu) c.fu = reinterpret_cast<float*>(ws + o.fu);
  return c;
}

// what every beam search's entry point is given; fn = its name, for the messages
struct SearchArgs {
  const char* fn;
  const float *x, *xproj;
  const glass_decoder_weights* w;
  int B, k, T, D, C, L, eos;
  int* out_symbols; float* out_scores; int* out_lengths; float* out_path;
  void* workspace; int64_t workspace_bytes;
  hipStream_t stream;
};
static int no_check() { return GLASS_OK; }

// The host side of every beam search: the checks in the order the entry points promise (the search's limits, limits() = the
// family's own, B == 0, null pointers, pointers() = the family's own outputs and arrays, the workspace), the workspace carved
// and the state zeroed, then attention for step 0, max_len x (GRU launch, step kernel), and the final kernel.
//   make_step(p, c) -> step(int): the family's step launch (p, c outlive it); final(c): its final launch, named final_fn in
//   the message of a failed launch
template <class Limits, class Pointers, class MakeStep, class Final>
static int run_beam_search(const SearchArgs& a, BeamTables tables, const char* final_fn, Limits limits, Pointers pointers,
                           MakeStep make_step, Final final) {
  if (int rc = search_limits(a.fn, true, a.B, a.k, a.T, a.D, a.C, a.L)) return rc;
  if (int rc = limits()) return rc;
  if (a.B == 0) return GLASS_OK;
  GLASS_CHECK_ARG(a.x && a.xproj && a.w && a.out_symbols && a.out_scores && a.out_lengths && a.workspace, "%s: null pointer", a.fn);
  if (int rc = pointers()) return rc;
  const BeamLayout lay = beam_layout(a.B, a.k, a.D, a.L, tables);
  GLASS_CHECK_ARG(a.workspace_bytes >= (int64_t)lay.total, "%s: workspace too small (%lld < %lld bytes)", a.fn,
                  (long long)a.workspace_bytes, (long long)lay.total);
  DecParams p = dec_params(a.x, a.xproj, a.w, a.B * a.k, a.T, a.C, a.L);
  const BeamCarved c = beam_carve(a.workspace, lay, tables, a.k, a.L, a.eos, p);
  hipError_t e = hipMemsetAsync(p.h0, 0, (size_t)a.B * a.k * a.D * sizeof(float), a.stream);  // initial state h = 0
  if (e != hipSuccess) { glass_set_error("%s: memset: %s", a.fn, hipGetErrorString(e)); return GLASS_EHIP; }
  auto step = make_step(p, c);
  step(-1);                                                                       // attention for step 0
  for (int t = 0; t < a.L; ++t) {
    dec_gru_step(p, p.h0, p.h1, a.stream);
    step(t);
  }
  GLASS_CHECK_LAUNCH(a.fn);
  final(c);
  GLASS_CHECK_LAUNCH(final_fn);
  return GLASS_OK;
}

// step == -1: only the attention part with h = 0, y = 0 ([GO]) -> inp rows of step 0; step >= 0: fc + log-softmax + running
// score + top-k of the item's k*C candidates -> tables[step], then (unless it is the last step) predecessor gather of the
// states and the attention / embedding part for step + 1.  The fc / sEmbed mat-vecs, the energies and the two reductions are
// dec_fc_att_kernel's, element for element, so the logits are those of glass_attention_decode_step on inflated inputs.
// KB = k rounded up to 1, 2, 4, 8 or 16 (rows >= k are zero and never written out).
template <int KB>
__global__ __launch_bounds__(256) void beam_step_kernel(DecParams p, BeamParams bp, const float* __restrict__ hraw, int step) {
  __shared__ __attribute__((aligned(16))) float h[KB][DEC_D];
  __shared__ __attribute__((aligned(16))) float sproj[KB][DEC_D];
  __shared__ float cand[KB][DEC_CMAX];
  __shared__ float energy[KB][DEC_TMAX];
  __shared__ float run[KB];
  __shared__ int ysel[KB], psel[KB];
  __shared__ float wbest[2][4];
  __shared__ int wbesti[2][4];
  const int u = threadIdx.x, b = blockIdx.x, lane = u & 63, wave = u >> 6;
  const int C = p.C, k = bp.k, L = bp.L;
  const long row0 = (long)b * k;
  rows_load<KB>(hraw, row0, k, step, u, h);
  if (u < KB) {
    ysel[u] = 0;
    psel[u] = 0;
    float rs = -INFINITY;
    if (u < k) {
      if (step <= 0) rs = u == 0 ? 0.f : -INFINITY;
      else {
        const long i = ((long)b * L + (step - 1)) * k + u;
        rs = bp.sy[i] == bp.eos ? -INFINITY : bp.sc[i];
      }
    }
    run[u] = rs;
  }
  __syncthreads();
  if (step >= 0) {
    rows_fc<KB>(p, C, u, h, cand);
    __syncthreads();
    rows_score<KB>(k, C, lane, wave, run, cand);
    __syncthreads();
    rows_topk<KB>(k, C, u, lane, wave, ~0u, cand, wbest, wbesti, [&](int j, float score, int beam, int cls) {
      const long i = ((long)b * L + step) * k + j;
      bp.sc[i] = score; bp.pr[i] = beam; bp.sy[i] = cls;
      ysel[j] = cls; psel[j] = beam;
    });
    if (step + 1 >= L) return;
    __syncthreads();
    rows_follow<KB>(k, row0, u, psel, h, bp.hsel);
  }
  rows_attend<KB>(p, b, k, row0, u, h, sproj, energy, ysel);
}

// rank of slot `i` among v[0..k) by value descending, then slot ascending (-inf entries last, in slot order)
__device__ __forceinline__ int beam_rank(const float* v, int k, int i) {
  int rank = 0;
  const float vi = v[i];
  for (int j = 0; j < k; ++j) rank += (v[j] > vi || (v[j] == vi && j < i)) ? 1 : 0;
  return rank;
}

// The reference's back-tracking (prediction_aster.py:161-222), one wavefront per item, lane r = result slot r: the last
// step's beams sorted, the backward pass with "an ended sequence replaces the worst slot" (slot k - found % k - 1, <eos>
// entries of a step taken from the highest beam down), the final re-sort.  Path rows of the best hypothesis: row t < length
// holds exp(score_t - score_{t-1}) at its symbol along the hypothesis's own ancestor chain, every other entry zero.
__global__ __launch_bounds__(64) void beam_backtrack_kernel(BeamParams bp, int C, int* __restrict__ out_sym,
                                                            float* __restrict__ out_sc, int* __restrict__ out_len,
                                                            float* __restrict__ out_path) {
  __shared__ int p_sym[BEAM_LMAX][BEAM_KMAX];
  __shared__ int p_idx[BEAM_LMAX][BEAM_KMAX];
  __shared__ float s_s[BEAM_KMAX];
  __shared__ int s_len[BEAM_KMAX], s_ord[BEAM_KMAX];
  const int b = blockIdx.x, lane = threadIdx.x, k = bp.k, L = bp.L;
  // the item's decision tables, staged once: the backward pass reads them in a dependent chain
  __shared__ float sc[BEAM_LMAX * BEAM_KMAX];
  __shared__ int pr[BEAM_LMAX * BEAM_KMAX], sy[BEAM_LMAX * BEAM_KMAX];
  for (int i = lane; i < L * k; i += 64) {
    sc[i] = bp.sc[(long)b * L * k + i];
    pr[i] = bp.pr[(long)b * L * k + i];
    sy[i] = bp.sy[(long)b * L * k + i];
  }
  __syncthreads();
  if (lane < k) s_s[lane] = sc[(L - 1) * k + lane];
  __syncthreads();
  if (lane < k) s_ord[beam_rank(s_s, k, lane)] = lane;
  __syncthreads();
  float s = 0.f;
  int tp = 0, len = L, found = 0;
  if (lane < k) { tp = s_ord[lane]; s = s_s[tp]; }
  for (int t = L - 1; t >= 0; --t) {
    int cur = 0, idx = 0;
    if (lane < k) { idx = tp; cur = sy[t * k + tp]; tp = pr[t * k + tp]; }
    for (int j = k - 1; j >= 0; --j) {
      const int symj = sy[t * k + j];
      if (symj == bp.eos) {
        const int res = k - (found % k) - 1;
        ++found;
        if (lane == res) { tp = pr[t * k + j]; cur = symj; idx = j; s = sc[t * k + j]; len = t + 1; }
      }
    }
    if (lane < k) { p_sym[t][lane] = cur; p_idx[t][lane] = idx; }
  }
  __syncthreads();
  if (lane < k) { s_s[lane] = s; s_len[lane] = len; }
  __syncthreads();
  if (lane < k) s_ord[beam_rank(s_s, k, lane)] = lane;
  __syncthreads();
  for (int i = lane; i < k * L; i += 64) {
    const int r = i / L, t = i - r * L;
    out_sym[((long)b * k + r) * L + t] = p_sym[t][s_ord[r]];
  }
  if (lane < k) {
    out_sc[(long)b * k + lane] = s_s[s_ord[lane]];
    out_len[(long)b * k + lane] = s_len[s_ord[lane]];
  }
  if (out_path == nullptr) return;
  float* op = out_path + (long)b * L * C;
  for (int i = lane; i < L * C; i += 64) op[i] = 0.f;
  __syncthreads();
  const int slot = s_ord[0];
  if (lane < s_len[slot] && s_s[slot] > -INFINITY) {
    const int t = lane;
    const float cur = sc[t * k + p_idx[t][slot]];
    const float prev = t > 0 ? sc[(t - 1) * k + p_idx[t - 1][slot]] : 0.f;
    op[(long)t * C + p_sym[t][slot]] = expf(cur - prev);
  }
}

extern "C" int64_t glass_beam_search_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  (void)T; (void)C;
  return (int64_t)beam_layout(B, k, D, max_len, BEAM_PLAIN).total;
}

extern "C" int glass_beam_search(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                                 int C, int max_len, int eos, int* out_symbols, float* out_scores, int* out_lengths,
                                 float* out_path_probs, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores, out_lengths,
                        out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  return run_beam_search(
      a, BEAM_PLAIN, "glass_beam_search(backtrack)", no_check, no_check,
      [&](const DecParams& p, const BeamCarved& c) {
        return [&](int step) {
          with_row_block(a.k, [&](auto kb) {
            hipLaunchKernelGGL(beam_step_kernel<decltype(kb)::value>, dim3(a.B), dim3(256), 0, a.stream, p, c.bp, p.h1, step);
          });
        };
      },
      [&](const BeamCarved& c) {
        hipLaunchKernelGGL(beam_backtrack_kernel, dim3(a.B), dim3(64), 0, a.stream, c.bp, C, out_symbols, out_scores, out_lengths,
                           out_path_probs);
      });
}

// ================================================================== forced decoding (AttentionRecognitionHead.forward)
// The decoder with the emitted symbols GIVEN (reference prediction_aster.py:33-60, teacher forcing): n sequences per item
// that share the item's x / xproj rows - a word to score, the k hypotheses of a beam search, lexicon candidates.  Per step
// dec_gru_kernel on the B*n state rows (ping-pong h0 / h1) and forced_step_kernel (one workgroup per item): fc, log-softmax,
// the records of the step, then attention + embedding of the given symbol for the next step.  No host synchronisation.
//   workspace: h0 [B*n,D] | h1 [B*n,D] | inp [B*n,2D] | effective length, bad-symbol flag [B*n] each
// A sequence is computed for t < its effective length; the GRU still runs on every row (rows past their length carry
// finite junk that is never written out).  A workgroup whose n sequences have all ended only writes the step's zeros.
struct ForcedParams {
  const int* targets;               // [B][n][L]
  const int* lengths;               // [B][n] or null
  float* step_logp;                 // [B][n][L]
  float* scores;                    // [B][n]: the running score between the launches, the result after the last one
  int* out_len;                     // [B][n]
  float* probs;                     // [B][n][L][C] or null
  float* logits;                    // [B][n][L][C] or null
  int* elen;                        // workspace [B*n]: number of steps computed
  int* bad;                         // workspace [B*n]: 1 = the sequence stopped at a symbol outside [0, C)
  int n, L, eos;
};
// what forced_step_kernel<KB, true> (glass_forced_attention) writes besides: a struct of its own and the kernel's LAST argument, so
// that the ATT = false kernel finds every other argument where it was
struct ForcedAttention {
  float* rows;                      // [B][n][L][T], cleared by the host; row t = the weights that made the context of step t
};

// step == -1: effective lengths from `lengths` or the first <eos>, scores = 0, and the attention part with h = 0, y = 0 ([GO])
// -> inp rows of step 0; step >= 0: fc + log-softmax of the GRU's output rows -> the records of row `step` (zeros for a
// sequence that has ended), then - if any sequence goes on - attention with y = targets[step] -> inp rows of step + 1.
// A symbol is used as an index (embedding row, log-softmax entry) only after the range check of the step -1 launch, which ends a
// sequence AT the first symbol outside [0, C) with score -inf; the index is clamped once more where it is used.
// ATT (glass_forced_attention, glass_hip_feature_chars.h): after the attention part, the weights it left in `energy` go to row
// step + 1 of every sequence that goes on to that step (one writer per element); all of it is under `if constexpr (ATT)`: the
// ATT = false kernel is the code it was.
template <int KB, bool ATT>
__global__ __launch_bounds__(256) void forced_step_kernel(DecParams p, ForcedParams fp, const float* __restrict__ hraw, int step,
                                                          ForcedAttention fa) {
  __shared__ __attribute__((aligned(16))) float h[KB][DEC_D];
  __shared__ __attribute__((aligned(16))) float sproj[KB][DEC_D];
  __shared__ float cand[KB][DEC_CMAX];
  __shared__ float energy[KB][DEC_TMAX];
  __shared__ int ycur[KB], ysel[KB], slen[KB], sbad[KB];
  const int u = threadIdx.x, lane = u & 63, wave = u >> 6;
  const int b = blockIdx.x;
  const int C = p.C, n = fp.n, L = fp.L;
  const long row0 = (long)b * n;
  if (u < KB) {
    int len = 0, bad = 0, y = 0;
    if (u < n) {
      const long row = row0 + u;
      const int* tg = fp.targets + row * L;
      if (step < 0) {
        const bool given = fp.lengths != nullptr;
        const int lim = given ? min(max(fp.lengths[row], 0), L) : L;
        len = lim;
        for (int t = 0; t < lim; ++t) {
          const int sym = tg[t];
          if (sym < 0 || sym >= C) { len = t; bad = 1; break; }
          if (!given && sym == fp.eos) { len = t + 1; break; }
        }
        fp.elen[row] = len;
        fp.bad[row] = bad;
        fp.out_len[row] = len;
        fp.scores[row] = (bad && len == 0) ? -INFINITY : 0.f;
      } else {
        len = fp.elen[row];
        bad = fp.bad[row];
        if (step < len) y = min(max(tg[step], 0), C - 1);
      }
    }
    ycur[u] = y;
    ysel[u] = (step >= 0 && step + 1 < len) ? y : 0;
    slen[u] = len;
    sbad[u] = bad;
  }
  __syncthreads();
  if (step >= 0) {
    bool now = false, next = false;
    for (int r = 0; r < n; ++r) { now = now || step < slen[r]; next = next || step + 1 < slen[r]; }
    if (now) {                                                  // uniform over the workgroup
#pragma unroll
      for (int r = 0; r < KB; ++r) h[r][u] = r < n ? hraw[(row0 + r) * DEC_D + u] : 0.f;
      __syncthreads();
      rows_fc<KB>(p, C, u, h, cand);
      __syncthreads();
    }
    // ---- the records of row `step`, wavefront per sequence
    for (int r = wave; r < n; r += 4) {
      const long rec = (row0 + r) * L + step;
      const bool live = step < slen[r];
      float v[DEC_CMAX / 64];
      float m = 0.f, ls = 0.f;
      if (live) ls = row_lsm(cand[r], C, lane, v, m);
#pragma unroll
      for (int i = 0; i < DEC_CMAX / 64; ++i) {
        const int cidx = lane + 64 * i;
        if (cidx < C) {
          const float l = live ? (v[i] - m) - ls : 0.f;
          if (fp.probs != nullptr) fp.probs[rec * C + cidx] = live ? expf(l) : 0.f;
          if (fp.logits != nullptr) fp.logits[rec * C + cidx] = live ? v[i] : 0.f;
          if (live && cidx == ycur[r]) {
            fp.step_logp[rec] = l;
            const float sc = fp.scores[row0 + r] + l;           // fl32(score_{t-1} + step_logp[t]), in step order
            fp.scores[row0 + r] = (sbad[r] && step + 1 == slen[r]) ? -INFINITY : sc;
          }
        }
      }
      if (!live && lane == 0) fp.step_logp[rec] = 0.f;
    }
    if (!next || step + 1 >= L) return;
    __syncthreads();
  } else {
#pragma unroll
    for (int r = 0; r < KB; ++r) h[r][u] = 0.f;
    __syncthreads();
  }
  rows_attend<KB>(p, b, n, row0, u, h, sproj, energy, ysel);
  if constexpr (ATT) {
    __syncthreads();
    const int T = p.T, at = step + 1;                           // at < L: the launch of step L - 1 has returned above
    for (int i = u; i < n * T; i += 256) {
      const int r = i / T, t = i - r * T;
      if (at < slen[r]) fa.rows[((row0 + r) * L + at) * T + t] = energy[r][t];
    }
  }
}

// the workspace as byte offsets and its size, for glass_forced_decode_workspace_bytes and the entry point alike
struct ForcedLayout { size_t h0, h1, inp, elen, bad, total; };
static ForcedLayout forced_layout(int B, int n, int D, int L) {
  if (B <= 0 || n <= 0 || D <= 0 || L <= 0) return {};
  const size_t rows = (size_t)B * n, state = rows * D * sizeof(float);
  return {0, state, 2 * state, 4 * state, 4 * state + rows * sizeof(int), 4 * state + 2 * rows * sizeof(int)};
}

extern "C" int64_t glass_forced_decode_workspace_bytes(int B, int n, int T, int D, int C, int max_len) {
  (void)T; (void)C;
  return (int64_t)forced_layout(B, n, D, max_len).total;
}

// the host side of glass_forced_decode (attention == nullptr: the ATT = false kernels) and of glass_forced_attention (the
// ATT = true kernels, the rows cleared by a memset first); fn = the entry's name, for the messages
static int run_forced(const char* fn, bool att, const float* x, const float* xproj, const glass_decoder_weights* w, int B, int n,
                      int T, int D, int C, int max_len, int eos, const int* targets, const int* lengths, float* out_step_logp,
                      float* out_scores, int* out_lengths, float* out_probs, float* out_logits, float* attention, void* workspace,
                      int64_t workspace_bytes, glass_stream_t stream) {
  if (int rc = search_limits(fn, false, B, n, T, D, C, max_len)) return rc;
  if (B == 0) return GLASS_OK;
  GLASS_CHECK_ARG(x && xproj && w && targets && out_step_logp && out_scores && out_lengths && workspace && (!att || attention),
                  "%s: null pointer", fn);
  const ForcedLayout lay = forced_layout(B, n, D, max_len);
  GLASS_CHECK_ARG(workspace_bytes >= (int64_t)lay.total, "%s: workspace too small (%lld < %lld bytes)", fn,
                  (long long)workspace_bytes, (long long)lay.total);
  hipStream_t s = (hipStream_t)stream;
  DecParams p = dec_params(x, xproj, w, B * n, T, C, max_len);
  char* ws = static_cast<char*>(workspace);
  p.h0 = reinterpret_cast<float*>(ws + lay.h0); p.h1 = reinterpret_cast<float*>(ws + lay.h1); p.inp = reinterpret_cast<float*>(ws + lay.inp);
  ForcedParams fp;
  fp.targets = targets; fp.lengths = lengths; fp.step_logp = out_step_logp; fp.scores = out_scores; fp.out_len = out_lengths;
  fp.probs = out_probs; fp.logits = out_logits;
  fp.elen = reinterpret_cast<int*>(ws + lay.elen); fp.bad = reinterpret_cast<int*>(ws + lay.bad);
  fp.n = n; fp.L = max_len; fp.eos = eos;
  const ForcedAttention fa = {att ? attention : nullptr};
  hipError_t e = hipMemsetAsync(p.h0, 0, lay.h1 - lay.h0, s);                      // initial state h = 0
  if (e == hipSuccess && att) e = hipMemsetAsync(attention, 0, (size_t)B * n * max_len * T * sizeof(float), s);
  if (e != hipSuccess) { glass_set_error("%s: memset: %s", fn, hipGetErrorString(e)); return GLASS_EHIP; }
  const dim3 gb(B);
  float* hb[2] = {p.h0, p.h1};
  auto forced_step = [&](const float* hraw, int step) {
    with_row_block(n, [&](auto kb) {
      constexpr int KB = decltype(kb)::value;
      if (att) hipLaunchKernelGGL((forced_step_kernel<KB, true>), gb, dim3(256), 0, s, p, fp, hraw, step, fa);
      else hipLaunchKernelGGL((forced_step_kernel<KB, false>), gb, dim3(256), 0, s, p, fp, hraw, step, fa);
    });
  };
  forced_step(hb[0], -1);                                                         // lengths, and the attention for step 0
  for (int step = 0; step < max_len; ++step) {
    dec_gru_step(p, hb[step & 1], hb[(step + 1) & 1], s);
    forced_step(hb[(step + 1) & 1], step);
  }
  GLASS_CHECK_LAUNCH(fn);
  return GLASS_OK;
}

extern "C" int glass_forced_decode(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int n, int T, int D,
                                   int C, int max_len, int eos, const int* targets, const int* lengths, float* out_step_logp,
                                   float* out_scores, int* out_lengths, float* out_probs, float* out_logits, void* workspace,
                                   int64_t workspace_bytes, glass_stream_t stream) {
  return run_forced("glass_forced_decode", false, x, xproj, w, B, n, T, D, C, max_len, eos, targets, lengths, out_step_logp,
                    out_scores, out_lengths, out_probs, out_logits, nullptr, workspace, workspace_bytes, stream);
}

// glass_hip_feature_chars.h: glass_forced_decode, and the attention rows [B][n][L][T] that formed each step's context
extern "C" int64_t glass_forced_attention_workspace_bytes(int B, int n, int T, int D, int C, int max_len) {
  return glass_forced_decode_workspace_bytes(B, n, T, D, C, max_len);
}

extern "C" int glass_forced_attention(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int n, int T,
                                      int D, int C, int max_len, int eos, const int* targets, const int* lengths,
                                      float* out_step_logp, float* out_scores, int* out_lengths, float* out_probs,
                                      float* out_logits, float* out_attention, void* workspace, int64_t workspace_bytes,
                                      glass_stream_t stream) {
  return run_forced("glass_forced_attention", true, x, xproj, w, B, n, T, D, C, max_len, eos, targets, lengths, out_step_logp,
                    out_scores, out_lengths, out_probs, out_logits, out_attention, workspace, workspace_bytes, stream);
}

// ================================================================== lexicon-constrained beam search (glass_hip_ext.h)
// glass_beam_search with a mask: every slot carries a node of the lexicon's trie, a candidate (beam, class) keeps its score
// only where the node has a child for the class's fold symbol (or, for <eos>, where a word ends at the node), and the
// finalisation returns the k best COMPLETED words.  The step is the unconstrained search's: the same rows_* pieces (the top-k with
// the mask as its `allow` bits) and the same GRU launch.
//   workspace: that of glass_beam_search | node table [B,L,k] (the slot's node after the step; -1 = dead)
struct LexParams {
  const unsigned* child_mask;       // [N][MW]
  const int* child_base;            // [N]
  const int* node_word;             // [N]
  const int* seg_root;              // [S]
  const int* fold;                  // [C]
  const int* item_segment;          // [B]
  int* nd;                          // workspace [B][L][k]
  int N, S, F, MW;
  static constexpr bool weighted = false;
  // ---- what con_step_kernel asks of a constraint (DfaParams answers the same questions from its table)
  // the node of an item's first beam; the caller checks it against N
  __device__ __forceinline__ int root(int b) const {
    const int seg = item_segment[b];
    return (seg >= 0 && seg < S) ? seg_root[seg] : -1;
  }
  // may a beam at `node` (inside [0,N)) emit the class: `stop` = it is <eos>, else `sym` = its fold symbol f is inside [0,F)
  __device__ __forceinline__ unsigned allow_bit(bool stop, bool sym, int f, int node, int step, int L) const {
    (void)step; (void)L;
    unsigned bit = 0u;
    if (stop) bit = node_word[node] >= 0 ? 1u : 0u;
    else if (sym) bit = (child_mask[(long)node * MW + (f >> 5)] >> (f & 31)) & 1u;
    return bit;
  }
  // the node after fold symbol f (inside [0,F)) from `par` (inside [0,N)); -1 for one outside the arrays
  __device__ __forceinline__ int follow(int par, int f) const {
    const unsigned* mw = child_mask + (long)par * MW;
    const int wq = f >> 5;
    int below = 0;
    for (int q = 0; q < wq; ++q) below += __popc(mw[q]);
    below += __popc(mw[wq] & ((1u << (f & 31)) - 1u));
    const long child = (long)child_base[par] + below;
    return (child >= 0 && child < N) ? (int)child : -1;
  }
};

// The constraint of glass_beam_search_dfa (glass_hip_feature_dfa.h): a slot's node is a state of the automaton
struct DfaParams {
  const int* next;                  // [N][F]: -1, or target | min(dist[target], 127) << 24
  const int* accept;                // [N]
  const int* start;                 // [S]
  const int* fold;                  // [C]
  const int* item_segment;          // [B]
  int* nd;                          // workspace [B][L][k]
  int N, S, F;
  static constexpr bool weighted = false;
  __device__ __forceinline__ int root(int b) const {
    const int seg = item_segment[b];
    return (seg >= 0 && seg < S) ? start[seg] : -1;
  }
  // one load decides a symbol: the transition exists and the string can still be completed, its stop at step L - 1 at the
  // latest.  The stop itself needs an accepting state and a non-empty string.
  __device__ __forceinline__ unsigned allow_bit(bool stop, bool sym, int f, int node, int step, int L) const {
    unsigned bit = 0u;
    if (stop) bit = (step >= 1 && accept[node] >= 0) ? 1u : 0u;
    else if (sym) {
      const int e = next[(long)node * F + f];
      bit = (e >= 0 && step + 1 + (e >> 24) <= L - 1) ? 1u : 0u;
    }
    return bit;
  }
  __device__ __forceinline__ int follow(int par, int f) const {
    const int e = next[(long)par * F + f];
    const int q = e & 0xffffff;
    return (e >= 0 && q < N) ? q : -1;
  }
};

// The constraint of glass_beam_search_wdfa (glass_hip_feature_wdfa.h): DfaParams with a weight on every transition, stop and
// start.  `weighted` switches con_step_kernel to two scores per slot: the model score (bp.sc, the arithmetic of the other
// searches) and the weight sum (wa); the beams are ranked by fuse(model score, weight sum) (fu).
struct WdfaParams {
  const unsigned long long* trans;  // [N][F]: next as in DfaParams in the low half, the float weight in the high half: read as
                                    // ONE 64-bit integer (two ints of a struct or an int2 become two dependent 32-bit loads)
  const float* final_w;             // [N]
  const float* start_w;             // [S]
  const int* accept;                // [N]
  const int* start;                 // [S]
  const int* fold;                  // [C]
  const int* item_segment;          // [B]
  int* nd;                          // workspace [B][L][k]
  float* wa;                        // workspace [B][L][k]: the slot's weight sum after the step
  float* fu;                        // workspace [B][L][k]: the slot's fused score after the step
  float scale;
  int N, S, F;
  static constexpr bool weighted = true;
  __device__ __forceinline__ int root(int b) const {
    const int seg = item_segment[b];
    return (seg >= 0 && seg < S) ? start[seg] : -1;
  }
  // the weight sum an item starts with (root(b) has checked the segment)
  __device__ __forceinline__ float root_weight(int b) const { return start_w[item_segment[b]]; }
  // ONE rounding: the product is not rounded on its own (scale = 0 or a = 0 give m bit for bit)
  __device__ __forceinline__ float fuse(float m, float a) const { return __fmaf_rn(scale, a, m); }
  // allow_bit of DfaParams with the weight: `a` = the beam's weight sum -> `term` = the candidate's; one 64-bit load decides a
  // symbol and weighs it.  A weight (or a sum) that is not finite: the candidate is absent.
  __device__ __forceinline__ unsigned allow_term(bool stop, bool sym, int f, int node, int step, int L, float a, float& term) const {
    bool ok = false;
    float w = 0.f;
    if (stop) {
      ok = step >= 1 && accept[node] >= 0;
      w = final_w[node];
    } else if (sym) {
      const unsigned long long e = trans[(long)node * F + f];
      const int nx = (int)(unsigned)e;
      ok = nx >= 0 && step + 1 + (nx >> 24) <= L - 1;
      w = __uint_as_float((unsigned)(e >> 32));
    }
    term = a + w;
    return (ok && fabsf(term) < INFINITY) ? 1u : 0u;
  }
  // follow of DfaParams, and the weight of the transition
  __device__ __forceinline__ int follow(int par, int f, float& w) const {
    const unsigned long long e = trans[(long)par * F + f];
    const int nx = (int)(unsigned)e, q = nx & 0xffffff;
    w = __uint_as_float((unsigned)(e >> 32));
    return (nx >= 0 && q < N) ? q : -1;
  }
};

// A constraint with the fold groups of a merged search (glass_hip_feature_merged.h): the classes of fold symbol f are
// group_cls[group_start[f] .. group_start[f + 1]), ascending.  What con_step_kernel<KB, Merged<CP>, true> reads next to CP's own.
template <class CP>
struct Merged : CP {
  const int* group_start;           // [F + 1]
  const int* group_cls;             // [n_group_cls]
  int n_group_cls;
};

// beam_step_kernel with the mask of a constraint CP (LexParams: the trie, DfaParams: the automaton, WdfaParams: the weighted
// automaton, whose extra work is all under `if constexpr (CP::weighted)`: the other two kernels are what they were).  Thread u
// owns class u: its k mask words or table entries (one per beam) are loaded once per step into the bit set `allow`; the k
// node ids live in LDS.  After the selection, thread j moves slot j to its child node / target state.
// MERGE (CP = Merged<...>): between the running scores and the top-k, the candidates of one beam whose classes share a fold
// symbol become ONE candidate - the group's arg-max class (ties: the lowest) carries the log of the group's summed mass, the
// other members lose their `allow` bit; the merged scores pass through sproj (idle at that point), so cand needs no second
// copy.  All of it is under `if constexpr (MERGE)`: the unmerged kernels are the code they were.
template <int KB, class CP, bool MERGE = false>
__global__ __launch_bounds__(256) void con_step_kernel(DecParams p, BeamParams bp, CP lp, const float* __restrict__ hraw,
                                                       int step) {
  __shared__ __attribute__((aligned(16))) float h[KB][DEC_D];
  __shared__ __attribute__((aligned(16))) float sproj[KB][DEC_D];
  __shared__ float cand[KB][DEC_CMAX];
  __shared__ float energy[KB][DEC_TMAX];
  __shared__ float run[KB], ssel[KB];
  __shared__ float arun[KB];                                            // weighted only: the slots' weight sums
  __shared__ int ysel[KB], psel[KB], snode[KB];
  __shared__ float wbest[2][4];
  __shared__ int wbesti[2][4];
  const int u = threadIdx.x, b = blockIdx.x, lane = u & 63, wave = u >> 6;
  const int C = p.C, k = bp.k, L = bp.L;
  const long row0 = (long)b * k;
  rows_load<KB>(hraw, row0, k, step, u, h);
  if (u < KB) {
    ysel[u] = 0;
    psel[u] = 0;
    ssel[u] = -INFINITY;
    float rs = -INFINITY;
    float ws = 0.f;
    int node = -1;
    if (u < k) {
      if (step <= 0) {
        if (u == 0) {
          rs = 0.f;
          node = lp.root(b);
          if constexpr (CP::weighted) {
            if (node >= 0) ws = lp.root_weight(b);
          }
        }
      } else {
        const long i = ((long)b * L + (step - 1)) * k + u;
        rs = bp.sc[i];
        node = bp.sy[i] == bp.eos ? -1 : lp.nd[i];
        if constexpr (CP::weighted) ws = lp.wa[i];
      }
      if constexpr (CP::weighted) {
        if (!(fabsf(ws) < INFINITY)) node = -1;                         // nothing is ranked by a weight that is not finite
      }
      if (node < 0 || node >= lp.N) { node = -1; rs = -INFINITY; }      // a dead slot: no node, never finite again
    }
    run[u] = rs;
    snode[u] = node;
    if constexpr (CP::weighted) arun[u] = node >= 0 ? ws : 0.f;
  }
  __syncthreads();
  if (step >= 0) {
    // ---- the mask of class u against the k nodes: bit r of `allow` = candidate (beam r, class u) may be emitted
    // (weighted: term[r] = the weight sum of that candidate, next to its bit)
    unsigned allow = 0u;
    float term[CP::weighted ? KB : 1];
    if constexpr (CP::weighted) {
#pragma unroll
      for (int r = 0; r < KB; ++r) term[r] = 0.f;
    }
    if constexpr (!CP::weighted) {
      if (u < C) {
        const bool stop = u == bp.eos;
        const int f = lp.fold[u];
        const bool sym = !stop && f >= 0 && f < lp.F;
#pragma unroll
        for (int r = 0; r < KB; ++r) {
          const int node = r < k ? snode[r] : -1;
          if (node >= 0) allow |= lp.allow_bit(stop, sym, f, node, step, L) << r;
        }
      }
    }
    rows_fc<KB>(p, C, u, h, cand);
    if constexpr (CP::weighted) {
      // after the mat-vec, not before it as the masks above: k weight terms alive across it cost the KB = 8 and 16 kernels 8
      // VGPRs (171 / 170 instead of 163 / 162) and with them a wave per SIMD; the loads still overlap the log-softmax
      if (u < C) {
        const bool stop = u == bp.eos;
        const int f = lp.fold[u];
        const bool sym = !stop && f >= 0 && f < lp.F;
#pragma unroll
        for (int r = 0; r < KB; ++r) {
          const int node = r < k ? snode[r] : -1;
          if (node >= 0) allow |= lp.allow_term(stop, sym, f, node, step, L, arun[r], term[r]) << r;
        }
      }
    }
    // MERGE: thread u's group [g0, g1) of group_cls, loaded here so that the loads overlap the log-softmax; left empty for the
    // stop, a class without a fold symbol, a one-class group (its candidate stays bit for bit) and a range outside the array.
    // c0, c1: the members of a group of two (a letter's two cases), kept in registers; a larger group is re-read row by row.
    // Every entry is range-checked before it indexes cand.
    [[maybe_unused]] int g0 = 0, g1 = 0, c0 = -1, c1 = -1;
    if constexpr (MERGE) {
      if (u < C && u != bp.eos) {
        const int f = lp.fold[u];
        if (f >= 0 && f < lp.F) {
          const int a = lp.group_start[f], e = lp.group_start[f + 1];
          if (a >= 0 && e <= lp.n_group_cls && e - a >= 2) {
            g0 = a; g1 = e;
            if (e - a == 2) { c0 = lp.group_cls[a]; c1 = lp.group_cls[a + 1]; }
          }
        }
      }
    }
    __syncthreads();
    rows_score<KB>(k, C, lane, wave, run, cand);
    __syncthreads();
    if constexpr (MERGE) {
      // every member reads its rows (is it the arg-max?  then the sum, in ascending class order) and parks the merged score in
      // sproj, which is idle until rows_attend; ONE barrier; only then the representatives overwrite their cells - cells the
      // other members have read to decide.  Nothing but the flags `rep` lives across the barrier.
      const bool pair = g1 - g0 == 2;
      unsigned rep = 0u;
#pragma unroll
      for (int r = 0; r < KB; ++r) {
        if (r < k && g1 > g0) {
          float top = -INFINITY;
          int at = -1;
          for (int i = g0; i < g1; ++i) {
            const int c = pair ? (i == g0 ? c0 : c1) : lp.group_cls[i];
            if (c >= 0 && c < C) {
              const float v = cand[r][c];
              if (at < 0 || v > top) { top = v; at = c; }
            }
          }
          if (at == u) {
            float s = top;                                               // an all -inf group stays -inf
            if (top > -INFINITY) {
              float sum = 0.f;
              for (int i = g0; i < g1; ++i) {
                const int c = pair ? (i == g0 ? c0 : c1) : lp.group_cls[i];
                if (c >= 0 && c < C) sum += expf(cand[r][c] - top);      // a member at -inf adds 0
              }
              s = top + logf(sum);
            }
            sproj[r][u] = s;
            rep |= 1u << r;
          } else {
            allow &= ~(1u << r);
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < KB; ++r)
        if ((rep >> r) & 1u) cand[r][u] = sproj[r][u];
      // (no barrier: the top-k reads cand[r][u] in thread u only, which wrote it)
    }
    if constexpr (CP::weighted) {
      // cand stays the model candidates; the top-k ranks them fused with the thread's k weight terms
      rows_topk_by<KB>(k, C, u, lane, wave, allow, [&](int r) { return lp.fuse(cand[r][u], term[r]); }, wbest, wbesti,
                       [&](int j, float score, int beam, int cls) {
        const long i = ((long)b * L + step) * k + j;
        lp.fu[i] = score; bp.pr[i] = beam; bp.sy[i] = cls;
        ysel[j] = cls; psel[j] = beam; ssel[j] = score;
      });
    } else {
      rows_topk<KB>(k, C, u, lane, wave, allow, cand, wbest, wbesti, [&](int j, float score, int beam, int cls) {
        const long i = ((long)b * L + step) * k + j;
        bp.sc[i] = score; bp.pr[i] = beam; bp.sy[i] = cls;
        ysel[j] = cls; psel[j] = beam; ssel[j] = score;
      });
    }
    __syncthreads();
    // ---- slot j follows its symbol into the trie / automaton: the child node, the node itself for <eos> (the terminal node,
    // whose word the finalisation reports), no node for a selected -inf candidate or an index outside the arrays
    // (weighted: the slot's two scores too - the winner's exact model score from cand, and its weight sum by the addition the
    // candidate was ranked with, on the entry loaded once more)
    if (u < k) {
      const int cls = ysel[u], par = snode[psel[u]];
      int node = -1;
      float w = 0.f;
      if (ssel[u] > -INFINITY && par >= 0) {
        if (cls == bp.eos) {
          node = par;
          if constexpr (CP::weighted) w = lp.final_w[par];
        } else {
          const int f = lp.fold[cls];
          if constexpr (CP::weighted) {
            if (f >= 0 && f < lp.F) node = lp.follow(par, f, w);
          } else {
            if (f >= 0 && f < lp.F) node = lp.follow(par, f);
          }
        }
      }
      const long i = ((long)b * L + step) * k + u;
      lp.nd[i] = node;
      if constexpr (CP::weighted) {
        const bool fin = ssel[u] > -INFINITY && par >= 0;
        bp.sc[i] = fin ? cand[psel[u]][cls] : -INFINITY;
        lp.wa[i] = fin ? arun[psel[u]] + w : 0.f;
      }
    }
    if (step + 1 >= L) return;
    __syncthreads();
    rows_follow<KB>(k, row0, u, psel, h, bp.hsel);
  }
  rows_attend<KB>(p, b, k, row0, u, h, sproj, energy, ysel);
}

// what con_final_kernel reads of a constraint: the node table and the tag of a node (the trie's node_word, an automaton's accept)
struct FinalParams {
  const int* nd;                    // workspace [B][L][k]
  const int* tag;                   // [N]
  int N;
};

// The k best completed entries of one item, one wavefront per item: an entry (t, slot) is completed when its symbol is <eos>
// and its score finite; order = score descending, then flat index t*k + slot ascending (t, then slot).  Lane l owns the
// entries l + 64 i; k rounds of the wavefront arg-max, then lane r walks result r back through the predecessor table.
// W (the weighted search): the entries are ranked by their fused scores `fused` [B][L][k], which go to out_sc; the model scores
// (bp.sc) go to out_model and, as without W, make the path rows.
template <bool W>
__global__ __launch_bounds__(64) void con_final_kernel(BeamParams bp, FinalParams fp, int C, int* __restrict__ out_sym,
                                                       float* __restrict__ out_sc, int* __restrict__ out_len,
                                                       int* __restrict__ out_word, float* __restrict__ out_path,
                                                       const float* __restrict__ fused, float* __restrict__ out_model) {
  __shared__ float sc[BEAM_LMAX * BEAM_KMAX];
  __shared__ float fu[W ? BEAM_LMAX * BEAM_KMAX : 1];
  __shared__ int pr[BEAM_LMAX * BEAM_KMAX], sy[BEAM_LMAX * BEAM_KMAX], nd[BEAM_LMAX * BEAM_KMAX];
  __shared__ int res[BEAM_KMAX];
  __shared__ int p_idx[BEAM_LMAX];            // the slots of result 0 along its ancestor chain
  const int b = blockIdx.x, lane = threadIdx.x, k = bp.k, L = bp.L, n = L * k;
  for (int i = lane; i < n; i += 64) {
    sc[i] = bp.sc[(long)b * n + i];
    pr[i] = bp.pr[(long)b * n + i];
    sy[i] = bp.sy[(long)b * n + i];
    nd[i] = fp.nd[(long)b * n + i];
    if constexpr (W) fu[i] = fused[(long)b * n + i];
  }
  __syncthreads();
  unsigned taken = 0u;
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY;
    int besti = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < BEAM_LMAX * BEAM_KMAX / 64; ++i) {
      const int e = lane + 64 * i;
      if (e < n && !((taken >> i) & 1u) && sy[e] == bp.eos) {
        float v;
        if constexpr (W) v = fu[e];
        else v = sc[e];
        if (v > -INFINITY && v < INFINITY && (besti == 0x7fffffff || v > best)) { best = v; besti = e; }
      }
    }
    wave_argmax_first(best, besti);
    if (besti != 0x7fffffff && (besti & 63) == lane) taken |= 1u << (besti >> 6);
    if (lane == 0) res[j] = besti == 0x7fffffff ? -1 : besti;
  }
  __syncthreads();
  if (lane < k) {
    const long row = (long)b * k + lane;
    int* os = out_sym + row * L;
    const int e = res[lane];
    if (e < 0) {
      for (int t = 0; t < L; ++t) os[t] = bp.eos;
      out_sc[row] = -INFINITY;
      if constexpr (W) out_model[row] = -INFINITY;
      out_len[row] = 0;
      out_word[row] = -1;
    } else {
      const int t0 = e / k;
      int slot = e - t0 * k;
      const int node = nd[e];
      if constexpr (W) {
        out_sc[row] = fu[e];
        out_model[row] = sc[e];
      } else {
        out_sc[row] = sc[e];
      }
      out_len[row] = t0 + 1;
      out_word[row] = (node >= 0 && node < fp.N) ? fp.tag[node] : -1;
      for (int t = L - 1; t > t0; --t) os[t] = bp.eos;
      for (int t = t0; t >= 0; --t) {
        os[t] = sy[t * k + slot];
        if (lane == 0) p_idx[t] = slot;
        slot = min(max(pr[t * k + slot], 0), k - 1);
      }
    }
  }
  if (out_path == nullptr) return;
  float* op = out_path + (long)b * L * C;
  for (int i = lane; i < L * C; i += 64) op[i] = 0.f;
  __syncthreads();
  const int e0 = res[0];
  if (e0 >= 0 && lane <= e0 / k) {
    const int t = lane;
    const float cur = sc[t * k + p_idx[t]];
    const float prev = t > 0 ? sc[(t - 1) * k + p_idx[t - 1]] : 0.f;
    op[(long)t * C + sy[t * k + p_idx[t]]] = expf(cur - prev);
  }
}

// ---- host side of the constrained searches
// the fold groups of a merged search, checked as far as the host can without reading device memory
struct FoldGroups { const int* start; const int* cls; int n; };
static int merged_limits(const char* fn, const FoldGroups& g, int C) {
  GLASS_CHECK_ARG(g.start && g.cls, "%s: null group array", fn);
  GLASS_CHECK_ARG(g.n >= 1 && g.n <= C, "%s: needs 1<=n_group_cls<=C (got n_group_cls=%d C=%d)", fn, g.n, C);
  return GLASS_OK;
}
static int automaton_limits(const char* fn, int N, int S, int F) {
  GLASS_CHECK_ARG(N >= 1 && N < (1 << 24) && S >= 1 && F >= 1 && F <= 256, "%s: needs 1<=N<2^24, S>=1, 1<=F<=256 (got N=%d S=%d F=%d)",
                  fn, N, S, F);
  return GLASS_OK;
}

// step(int) of a search under constraint cp: con_step_kernel<KB, CP>, or with fold groups con_step_kernel<KB, Merged<CP>, true>.
// G = const FoldGroups* (null = unmerged), or std::nullptr_t for a constraint that is never merged (the trie), whose merged
// kernels then do not exist.
template <class CP, class G>
static auto con_stepper(const SearchArgs& a, const DecParams& p, const BeamParams& bp, const CP& cp, G groups) {
  Merged<CP> mp = {};                                                              // group_start stays null: unmerged
  static_cast<CP&>(mp) = cp;
  if constexpr (!std::is_null_pointer_v<G>)
    if (groups != nullptr) { mp.group_start = groups->start; mp.group_cls = groups->cls; mp.n_group_cls = groups->n; }
  return [&a, &p, &bp, mp](int step) {
    with_row_block(a.k, [&](auto kb) {
      constexpr int KB = decltype(kb)::value;
      const dim3 gb(a.B), tb(256);
      if constexpr (!std::is_null_pointer_v<G>) {
        if (mp.group_start != nullptr) {
          hipLaunchKernelGGL((con_step_kernel<KB, Merged<CP>, true>), gb, tb, 0, a.stream, p, bp, mp, p.h1, step);
          return;
        }
      }
      hipLaunchKernelGGL((con_step_kernel<KB, CP>), gb, tb, 0, a.stream, p, bp, static_cast<const CP&>(mp), p.h1, step);
    });
  };
}

// run_beam_search for constraint cp (its workspace tables are set here): `tag` [N] = what out_tags reports of a hypothesis's
// last node; out_model = the weighted search's model scores, else null
template <class CP, class G, class Limits, class Pointers>
static int con_search(const SearchArgs& a, const char* final_fn, CP cp, G groups, const int* tag, int* out_tags, float* out_model,
                      Limits limits, Pointers pointers) {
  return run_beam_search(
      a, CP::weighted ? BEAM_WEIGHTED : BEAM_NODES, final_fn, limits, pointers,
      [&](const DecParams& p, const BeamCarved& c) {
        cp.nd = c.nd;
        if constexpr (CP::weighted) { cp.wa = c.wa; cp.fu = c.fu; }
        return con_stepper(a, p, c.bp, cp, groups);
      },
      [&](const BeamCarved& c) {
        const FinalParams fin = {c.nd, tag, cp.N};
        hipLaunchKernelGGL(con_final_kernel<CP::weighted>, dim3(a.B), dim3(64), 0, a.stream, c.bp, fin, a.C, a.out_symbols,
                           a.out_scores, a.out_lengths, out_tags, a.out_path, (const float*)c.fu, out_model);
      });
}

extern "C" int64_t glass_beam_search_lexicon_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  (void)T; (void)C;
  return (int64_t)beam_layout(B, k, D, max_len, BEAM_NODES).total;
}

extern "C" int glass_beam_search_lexicon(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T,
                                         int D, int C, int max_len, int eos, const uint32_t* child_mask, const int* child_base,
                                         const int* node_word, const int* seg_root, const int* fold, int N, int S, int F,
                                         const int* item_segment, int* out_symbols, float* out_scores, int* out_lengths,
                                         int* out_words, float* out_path_probs, void* workspace, int64_t workspace_bytes,
                                         glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search_lexicon", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores, out_lengths,
                        out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  LexParams lp;
  lp.child_mask = child_mask; lp.child_base = child_base; lp.node_word = node_word; lp.seg_root = seg_root; lp.fold = fold;
  lp.item_segment = item_segment; lp.nd = nullptr;
  lp.N = N; lp.S = S; lp.F = F; lp.MW = (F + 31) / 32;
  return con_search(
      a, "glass_beam_search_lexicon(final)", lp, nullptr, node_word, out_words, (float*)nullptr,
      [&] {
        GLASS_CHECK_ARG(N >= 1 && S >= 1 && F >= 1 && F <= 256, "%s: needs N>=1, S>=1, 1<=F<=256 (got N=%d S=%d F=%d)", a.fn, N, S, F);
        return GLASS_OK;
      },
      [&] {
        GLASS_CHECK_ARG(out_words, "%s: null pointer", a.fn);
        GLASS_CHECK_ARG(child_mask && child_base && node_word && seg_root && fold && item_segment, "%s: null trie array", a.fn);
        return GLASS_OK;
      });
}

// ================================================================== pattern-constrained beam search (glass_hip_feature_dfa.h)
// glass_beam_search_lexicon with the trie generalised to a DFA over fold symbols: the same step kernel with DfaParams as its
// constraint, the same workspace, and con_final_kernel with `accept` as the tags.  The merged twin
// (glass_hip_feature_merged.h) is the same search with MERGE in its step kernel.
extern "C" int64_t glass_beam_search_dfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  return glass_beam_search_lexicon_workspace_bytes(B, k, T, D, C, max_len);
}
extern "C" int64_t glass_beam_search_merged_dfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  return glass_beam_search_lexicon_workspace_bytes(B, k, T, D, C, max_len);
}

// glass_beam_search_dfa (groups == nullptr) and glass_beam_search_merged_dfa
static int dfa_search(const SearchArgs& a, const FoldGroups* groups, const int* next, const int* accept, const int* start,
                      const int* fold, int N, int S, int F, const int* item_pattern, int* out_tags) {
  DfaParams dp;
  dp.next = next; dp.accept = accept; dp.start = start; dp.fold = fold; dp.item_segment = item_pattern; dp.nd = nullptr;
  dp.N = N; dp.S = S; dp.F = F;
  return con_search(
      a, a.fn, dp, groups, accept, out_tags, (float*)nullptr,
      [&] {
        if (int rc = automaton_limits(a.fn, N, S, F)) return rc;
        return groups != nullptr ? merged_limits(a.fn, *groups, a.C) : GLASS_OK;
      },
      [&] {
        GLASS_CHECK_ARG(out_tags, "%s: null pointer", a.fn);
        GLASS_CHECK_ARG(next && accept && start && fold && item_pattern, "%s: null automaton array", a.fn);
        return GLASS_OK;
      });
}

extern "C" int glass_beam_search_dfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                                     int C, int max_len, int eos, const int* next, const int* accept, const int* start,
                                     const int* fold, int N, int S, int F, const int* item_pattern, int* out_symbols,
                                     float* out_scores, int* out_lengths, int* out_tags, float* out_path_probs, void* workspace,
                                     int64_t workspace_bytes, glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search_dfa", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores, out_lengths,
                        out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  return dfa_search(a, nullptr, next, accept, start, fold, N, S, F, item_pattern, out_tags);
}

extern "C" int glass_beam_search_merged_dfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T,
                                            int D, int C, int max_len, int eos, const int* next, const int* accept, const int* start,
                                            const int* fold, int N, int S, int F, const int* item_pattern, const int* group_start,
                                            const int* group_cls, int n_group_cls, int* out_symbols, float* out_scores,
                                            int* out_lengths, int* out_tags, float* out_path_probs, void* workspace,
                                            int64_t workspace_bytes, glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search_merged_dfa", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores,
                        out_lengths, out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  const FoldGroups groups = {group_start, group_cls, n_group_cls};
  return dfa_search(a, &groups, next, accept, start, fold, N, S, F, item_pattern, out_tags);
}

// ================================================================== weighted-automaton beam search (glass_hip_feature_wdfa.h)
// glass_beam_search_dfa with a weight on every transition, stop and start: the same step kernel with WdfaParams as its
// constraint (two scores per slot, ranked by their fusion), con_final_kernel<true>, and the merged twin likewise.
//   workspace: that of glass_beam_search_dfa | weight sums [B,L,k] | fused scores [B,L,k]
extern "C" int64_t glass_beam_search_wdfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  (void)T; (void)C;
  return (int64_t)beam_layout(B, k, D, max_len, BEAM_WEIGHTED).total;
}
extern "C" int64_t glass_beam_search_merged_wdfa_workspace_bytes(int B, int k, int T, int D, int C, int max_len) {
  return glass_beam_search_wdfa_workspace_bytes(B, k, T, D, C, max_len);
}

// glass_beam_search_wdfa (groups == nullptr) and glass_beam_search_merged_wdfa
static int wdfa_search(const SearchArgs& a, const FoldGroups* groups, const glass_wdfa_transition* trans, const float* final_w,
                       const float* start_w, const int* accept, const int* start, const int* fold, int N, int S, int F,
                       const int* item_pattern, float weight_scale, float* out_model_scores, int* out_tags) {
  static_assert(sizeof(glass_wdfa_transition) == 8 && offsetof(glass_wdfa_transition, w) == 4, "one 64-bit load per table entry");
  WdfaParams wp;
  wp.trans = reinterpret_cast<const unsigned long long*>(trans); wp.final_w = final_w; wp.start_w = start_w; wp.accept = accept;
  wp.start = start; wp.fold = fold; wp.item_segment = item_pattern; wp.nd = nullptr; wp.wa = nullptr; wp.fu = nullptr;
  wp.scale = weight_scale; wp.N = N; wp.S = S; wp.F = F;
  return con_search(
      a, a.fn, wp, groups, accept, out_tags, out_model_scores,
      [&] {
        if (int rc = automaton_limits(a.fn, N, S, F)) return rc;
        GLASS_CHECK_ARG(weight_scale == weight_scale && weight_scale - weight_scale == 0.f, "%s: weight_scale must be finite (got %g)",
                        a.fn, (double)weight_scale);
        return groups != nullptr ? merged_limits(a.fn, *groups, a.C) : GLASS_OK;
      },
      [&] {
        GLASS_CHECK_ARG(out_model_scores && out_tags, "%s: null pointer", a.fn);
        GLASS_CHECK_ARG(trans && final_w && start_w && accept && start && fold && item_pattern, "%s: null automaton array", a.fn);
        GLASS_CHECK_ARG((reinterpret_cast<uintptr_t>(trans) & 7u) == 0, "%s: trans is not 8-byte aligned", a.fn);
        return GLASS_OK;
      });
}

extern "C" int glass_beam_search_wdfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T, int D,
                                      int C, int max_len, int eos, const glass_wdfa_transition* trans, const float* final_w,
                                      const float* start_w, const int* accept, const int* start, const int* fold, int N, int S,
                                      int F, const int* item_pattern, float weight_scale, int* out_symbols, float* out_scores,
                                      float* out_model_scores, int* out_lengths, int* out_tags, float* out_path_probs,
                                      void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search_wdfa", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores, out_lengths,
                        out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  return wdfa_search(a, nullptr, trans, final_w, start_w, accept, start, fold, N, S, F, item_pattern, weight_scale, out_model_scores,
                     out_tags);
}

extern "C" int glass_beam_search_merged_wdfa(const float* x, const float* xproj, const glass_decoder_weights* w, int B, int k, int T,
                                             int D, int C, int max_len, int eos, const glass_wdfa_transition* trans,
                                             const float* final_w, const float* start_w, const int* accept, const int* start,
                                             const int* fold, int N, int S, int F, const int* item_pattern, float weight_scale,
                                             const int* group_start, const int* group_cls, int n_group_cls, int* out_symbols,
                                             float* out_scores, float* out_model_scores, int* out_lengths, int* out_tags,
                                             float* out_path_probs, void* workspace, int64_t workspace_bytes,
                                             glass_stream_t stream) {
  const SearchArgs a = {"glass_beam_search_merged_wdfa", x, xproj, w, B, k, T, D, C, max_len, eos, out_symbols, out_scores,
                        out_lengths, out_path_probs, workspace, workspace_bytes, (hipStream_t)stream};
  const FoldGroups groups = {group_start, group_cls, n_group_cls};
  return wdfa_search(a, &groups, trans, final_w, start_w, accept, start, fold, N, S, F, item_pattern, weight_scale,
                     out_model_scores, out_tags);
}
