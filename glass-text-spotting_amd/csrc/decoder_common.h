// Shared by the attention-GRU decoder (decoder.hip: the greedy decode and the single step) and its searches
// (decoder_search.hip: beam search, forced decoding, the lexicon-, pattern- and weighted-pattern-constrained beam searches): limits, the kernel
// parameter block, the host helpers every entry point uses, and the pieces of one decoder step on the rows of ONE item.
#pragma once
#include "recognition_common.h"

constexpr int DEC_D = 256;
constexpr int DEC_TMAX = 64;
constexpr int DEC_CMAX = 256;
constexpr int BEAM_KMAX = 16;   // rows per item of a search: beams, or given sequences
constexpr int BEAM_LMAX = 64;

struct DecParams {
  const float* x; const float* xproj;
  const float *sW, *sB, *wW, *wB, *emb, *w_ih, *w_hh, *b_ih, *b_hh, *fcW, *fcB;
  float temperature;
  int R, T, C, max_len;
  float* out;
  int* pred;
  float* h0; float* h1; float* inp; int* yprev;     // workspace: state (double-buffered), [emb|ctx], last argmax
  float* logits;                                    // glass_attention_decode_step only: raw fc outputs [R, C] (else null)
};

// ---- host helpers, defined in decoder.hip
// the weight pointers and sizes filled in; every output / workspace pointer null: the entry point sets the ones its kernels use
DecParams dec_params(const float* x, const float* xproj, const glass_decoder_weights* w, int rows, int T, int C, int max_len);
// hnext = GRUCell(p.inp, hprev) on the p.R rows: the one launch of dec_gru_kernel (the library is built without relocatable
// device code, so the kernel is launched from its own translation unit only)
void dec_gru_step(const DecParams& p, const float* hprev, float* hnext, hipStream_t stream);

// ---- pieces of one decoder step on the KB rows of ONE item (beam_step_kernel / con_step_kernel: its k beams;
// forced_step_kernel: its n given sequences), called by all 256 threads of the workgroup; u = threadIdx.x, lane = u & 63,
// wave = u >> 6 (rows_score and rows_topk take the kernel's own lane / wave: deriving them again from u cost the KB = 4 kernels
// 55 VGPRs and a wave per SIMD).  The mat-vecs, the energies and the reductions are dec_fc_att_kernel's arithmetic, element
// for element.  KB = the row count rounded up to 1, 2, 4, 8 or 16 (rows beyond it are zero and never written out).
// the GRU's output rows of the item -> h (zeros before the first step, step < 0, and in the rows >= k)
template <int KB>
__device__ __forceinline__ void rows_load(const float* __restrict__ hraw, long row0, int k, int step, int u, float (&h)[KB][DEC_D]) {
#pragma unroll
  for (int r = 0; r < KB; ++r) h[r][u] = (step >= 0 && r < k) ? hraw[(row0 + r) * DEC_D + u] : 0.f;
}

// logits = fc(h) * temperature -> cand[r][0..C)
template <int KB>
__device__ __forceinline__ void rows_fc(const DecParams& p, int C, int u, const float (*h)[DEC_D], float (*cand)[DEC_CMAX]) {
  if (u < C) {
    float acc[1][KB];
#pragma unroll
    for (int r = 0; r < KB; ++r) acc[0][r] = p.fcB[u];
    stream_matvec<1, KB, 16>(reinterpret_cast<const float4*>(p.fcW), C, 0, u, DEC_D / 4, &h[0][0], DEC_D, acc);
#pragma unroll
    for (int r = 0; r < KB; ++r) cand[r][u] = acc[0][r] * p.temperature;
  }
}

// log-softmax of one row by one wavefront: lane owns classes lane + 64 i -> v[i] = x (-inf beyond C), m = max, returns
// log(sum exp(x - m)); the log-softmax of class lane + 64 i is (v[i] - m) - ls
__device__ __forceinline__ float row_lsm(const float* row, int C, int lane, float (&v)[DEC_CMAX / 64], float& m) {
  m = -INFINITY;
#pragma unroll
  for (int i = 0; i < DEC_CMAX / 64; ++i) {
    const int cidx = lane + 64 * i;
    v[i] = cidx < C ? row[cidx] : -INFINITY;
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < DEC_CMAX / 64; ++i) s += (lane + 64 * i) < C ? expf(v[i] - m) : 0.f;
  s = wave_sum(s);
  return logf(s);
}

// candidate score = running score + log-softmax (x - max - log(sum exp(x - max))), in place in cand; wavefront per beam
template <int KB>
__device__ __forceinline__ void rows_score(int k, int C, int lane, int wave, const float (&run)[KB], float (&cand)[KB][DEC_CMAX]) {
  for (int r = wave; r < k; r += 4) {
    float v[DEC_CMAX / 64];
    float m;
    const float ls = row_lsm(cand[r], C, lane, v, m), rs = run[r];
#pragma unroll
    for (int i = 0; i < DEC_CMAX / 64; ++i) {
      const int cidx = lane + 64 * i;
      if (cidx < C) cand[r][cidx] = rs + ((v[i] - m) - ls);
    }
  }
}

// top k of the item's k*C candidates: k rounds of (max score, then min flat index beam*C + class); thread u owns class u of
// every beam.  Bit r of the thread's `allow` = candidate (beam r, class u) keeps its score, else it counts as -inf (-inf
// candidates are selected last, in index order); the unconstrained search passes all ones.  Thread 0 hands round j's
// choice to emit(j, score, beam, class), which writes it where the kernel wants it.  The caller has synchronised after
// writing cand and synchronises before reading what emit wrote.
template <int KB, class Emit>
__device__ __forceinline__ void rows_topk(int k, int C, int u, int lane, int wave, unsigned allow, const float (&cand)[KB][DEC_CMAX],
                                          float (&wbest)[2][4], int (&wbesti)[2][4], Emit emit) {
  unsigned taken = 0u;
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY;
    int besti = 0x7fffffff;
    if (u < C) {
#pragma unroll
      for (int r = 0; r < KB; ++r) {
        if (r < k && !((taken >> r) & 1u)) {
          const float v = ((allow >> r) & 1u) ? cand[r][u] : -INFINITY;
          if (besti == 0x7fffffff || v > best) { best = v; besti = r * C + u; }
        }
      }
    }
    wave_argmax_first(best, besti);
    if (lane == 0) { wbest[j & 1][wave] = best; wbesti[j & 1][wave] = besti; }
    __syncthreads();
    float gb = wbest[j & 1][0];
    int gi = wbesti[j & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float vb = wbest[j & 1][w];
      const int vi = wbesti[j & 1][w];
      if (vi != 0x7fffffff && (gi == 0x7fffffff || vb > gb || (vb == gb && vi < gi))) { gb = vb; gi = vi; }
    }
    // k <= C: a candidate is always left and gi is a real index - unless the logits hold NaN (outside the contract):
    // the tables must still hold valid slots and classes, they index memory in the later steps and in the finalisation, and
    // a score that is a number: where all of wave 0's 64 lanes hold NaN so does its maximum gb, and beam_rank, which gives
    // every NaN rank 0, would leave result slots of the back-tracking unassigned
    if (gi == 0x7fffffff) { gi = j; gb = -INFINITY; }
    const int beam = gi / C, cls = gi - beam * C;
    if (u == cls) taken |= 1u << beam;
    if (u == 0) emit(j, gb, beam, cls);
  }
}

// rows_topk with the candidate's score from a callback: value(r) = thread u's score of (beam r, class u), asked only where the
// bit is set and u < C (the weighted search: cand[r][u] fused with the thread's weight term of beam r).  The same rounds, rule
// and emit; a copy, so that the kernels of the unweighted searches are the code they were.
template <int KB, class Value, class Emit>
__device__ __forceinline__ void rows_topk_by(int k, int C, int u, int lane, int wave, unsigned allow, Value value,
                                             float (&wbest)[2][4], int (&wbesti)[2][4], Emit emit) {
  unsigned taken = 0u;
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY;
    int besti = 0x7fffffff;
    if (u < C) {
#pragma unroll
      for (int r = 0; r < KB; ++r) {
        if (r < k && !((taken >> r) & 1u)) {
          const float v = ((allow >> r) & 1u) ? value(r) : -INFINITY;
          if (besti == 0x7fffffff || v > best) { best = v; besti = r * C + u; }
        }
      }
    }
    wave_argmax_first(best, besti);
    if (lane == 0) { wbest[j & 1][wave] = best; wbesti[j & 1][wave] = besti; }
    __syncthreads();
    float gb = wbest[j & 1][0];
    int gi = wbesti[j & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float vb = wbest[j & 1][w];
      const int vi = wbesti[j & 1][w];
      if (vi != 0x7fffffff && (gi == 0x7fffffff || vb > gb || (vb == gb && vi < gi))) { gb = vb; gi = vi; }
    }
    // k <= C: a candidate is always left and gi is a real index - unless the logits hold NaN (outside the contract):
    // the tables must still hold valid slots and classes, they index memory in the later steps and in the finalisation, and
    // a score that is a number: where all of wave 0's 64 lanes hold NaN so does its maximum gb, and beam_rank, which gives
    // every NaN rank 0, would leave result slots of the back-tracking unassigned
    if (gi == 0x7fffffff) { gi = j; gb = -INFINITY; }
    const int beam = gi / C, cls = gi - beam * C;
    if (u == cls) taken |= 1u << beam;
    if (u == 0) emit(j, gb, beam, cls);
  }
}

// the states follow their predecessors: h[r] = h[psel[r]] (in place: column u of every row passes through registers), also
// written to hsel, the GRU's h_prev of the next step.  The caller has synchronised after writing psel.
template <int KB>
__device__ __forceinline__ void rows_follow(int k, long row0, int u, const int (&psel)[KB], float (&h)[KB][DEC_D],
                                            float* hsel) {
  float hv[KB];
#pragma unroll
  for (int r = 0; r < KB; ++r) hv[r] = r < k ? h[psel[r]][u] : 0.f;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < KB; ++r) {
    h[r][u] = hv[r];
    if (r < k) hsel[(row0 + r) * DEC_D + u] = hv[r];
  }
  __syncthreads();
}

// additive attention of the item's k rows with the states in h, and the GRU input of the next step:
// inp[row0 + r] = [embedding(ysel[r]) | alpha[r] . x[b]] for r < k.  x / xproj rows of item b are read once and serve all k rows.
// The caller has synchronised after writing h and ysel.
template <int KB>
__device__ __forceinline__ void rows_attend(const DecParams& p, int b, int k, long row0, int u, const float (*h)[DEC_D],
                                            float (*sproj)[DEC_D], float (*energy)[DEC_TMAX], const int* ysel) {
  const int lane = u & 63, wave = u >> 6, T = p.T;
  // ---- sProj = sEmbed(h)
  {
    float acc[1][KB];
#pragma unroll
    for (int r = 0; r < KB; ++r) acc[0][r] = p.sB[u];
    stream_matvec<1, KB, 16>(reinterpret_cast<const float4*>(p.sW), DEC_D, 0, u, DEC_D / 4, &h[0][0], DEC_D, acc);
#pragma unroll
    for (int r = 0; r < KB; ++r) sproj[r][u] = acc[0][r];
  }
  __syncthreads();
  // ---- energies e[r][t] = wEmbed(tanh(sProj[r] + xProj[t])): one xProj row per wavefront pass, shared by the k rows
  {
    const float4 ww = *reinterpret_cast<const float4*>(p.wW + lane * 4);
    const float wb = p.wB[0];
    for (int t = wave; t < T; t += 4) {
      const float4 xp = *reinterpret_cast<const float4*>(p.xproj + ((long)b * T + t) * DEC_D + lane * 4);
      for (int r = 0; r < k; ++r) {
        const float4 sp = *reinterpret_cast<const float4*>(&sproj[r][lane * 4]);
        float s = ww.x * tanh_fast(sp.x + xp.x) + ww.y * tanh_fast(sp.y + xp.y) + ww.z * tanh_fast(sp.z + xp.z) +
                  ww.w * tanh_fast(sp.w + xp.w);
        s = wave_sum(s);
        if (lane == 0) energy[r][t] = s + wb;
      }
    }
  }
  __syncthreads();
  for (int r = wave; r < k; r += 4) {
    const float v = lane < T ? energy[r][lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < T ? expf(v - m) : 0.f;
    const float s = wave_sum(e);
    if (lane < T) energy[r][lane] = e / s;
  }
  __syncthreads();
  // ---- inp = [embedding(y) | context = alpha . x]: one x row per t, shared by the k rows
  {
    float s[KB];
#pragma unroll
    for (int r = 0; r < KB; ++r) s[r] = 0.f;
    const float* xr = p.x + (long)b * T * DEC_D + u;
    for (int t = 0; t < T; ++t) {
      const float xv = xr[(long)t * DEC_D];
#pragma unroll
      for (int r = 0; r < KB; ++r)
        if (r < k) s[r] += energy[r][t] * xv;
    }
#pragma unroll
    for (int r = 0; r < KB; ++r) {
      if (r < k) {
        float* ip = p.inp + (row0 + r) * (2 * DEC_D);
        ip[u] = p.emb[(long)ysel[r] * DEC_D + u];
        ip[DEC_D + u] = s[r];
      }
    }
  }
}
