// The greedy attention-GRU decoder of the per-RoI recognition head, independent across RoIs.
// Two launches per decoding step, issued back to back by the host function (no host sync, argmax feedback
// stays on device):
//   dec_fc_att_kernel  (4 RoIs per workgroup): [fc + softmax + argmax of the state h_i -> out[:, i], y_i]
//                       then [additive attention with h_i -> context, embedding(y_i)] -> inp_{i+1}
//   dec_gru_kernel     (16 RoIs x GRU_UB hidden units per workgroup): GRU cell on v_mfma_f32_16x16x4_f32,
//                       every workgroup streams only its 3*GRU_UB-row slice of W_ih / W_hh from L2.
// A persistent workgroup per RoI group has to pull all 2.6 MB of decoder weights through ONE CU per step
// (80 us/step measured); spreading each step over the chip costs two launch boundaries (~2 us each).
// Weights stream from L2 in a k-blocked layout (packed[k/4][row][4]) so that the 64 lanes of a wavefront read 1 KiB
// contiguous per load.  The searches over this decoder are in decoder_search.hip.
#include "decoder_common.h"

constexpr int GRU_RB = 16;
constexpr int GRU_UB = 16;      // hidden units per workgroup: 16 -> 16 x 16 = 256 workgroups at R = 256 (one per CU; 32 left half the chip idle)

// step == -1: only the attention part with the initial input (y = 0); step == -2: only the attention part with y read from
// p.yprev (one decoder step of a caller-driven search, glass_attention_decode_step); do_att == 0: only the fc part (last step)
// DEC_RB = RoIs per workgroup: 4 when there are enough RoIs to fill the chip with 4-RoI workgroups, else 2 or 1
// (R = 256: 64 workgroups of 4 leave 3/4 of the CUs idle for 38 us per step; 256 workgroups of 1 take 12 us).
template <int DEC_RB>
__global__ __launch_bounds__(256) void dec_fc_att_kernel(DecParams p, const float* __restrict__ hcur, int step, int do_att) {
  __shared__ __attribute__((aligned(16))) float h[DEC_RB][DEC_D];
  __shared__ float sproj[DEC_RB][DEC_D];
  __shared__ float energy[DEC_RB][DEC_TMAX];
  __shared__ float logit[DEC_RB][DEC_CMAX];
  __shared__ int ycur[DEC_RB];
  const int u = threadIdx.x, lane = u & 63, wave = u >> 6;
  const int r0 = blockIdx.x * DEC_RB;
  const int nr = min(DEC_RB, p.R - r0);
  const int T = p.T, C = p.C;
#pragma unroll
  for (int r = 0; r < DEC_RB; ++r) h[r][u] = (r < nr) ? hcur[(long)(r0 + r) * DEC_D + u] : 0.f;
  // previous symbol: 0 ([GO]) before the first step; not read at all by an fc-only launch (do_att == 0: the beam-search entry
  // points p.yprev at scratch it has not written yet); a caller-supplied symbol (glass_attention_decode_step) is clamped to
  // the embedding table - an index outside [0, C) must not become an out-of-bounds read behind a C ABI
  if (u < DEC_RB) ycur[u] = (step == -1 || u >= nr || !do_att) ? 0 : min(max(p.yprev[r0 + u], 0), C - 1);
  __syncthreads();
  if (step >= 0) {
    // ---- logits = fc(h) * temperature; softmax over C; argmax (first maximum)
    if (u < C) {
      float acc[1][DEC_RB];
#pragma unroll
      for (int r = 0; r < DEC_RB; ++r) acc[0][r] = p.fcB[u];
      stream_matvec<1, DEC_RB, 16>(reinterpret_cast<const float4*>(p.fcW), C, 0, u, DEC_D / 4, &h[0][0], DEC_D, acc);
#pragma unroll
      for (int r = 0; r < DEC_RB; ++r) {
        logit[r][u] = acc[0][r] * p.temperature;
        if (p.logits != nullptr && r < nr) p.logits[(long)(r0 + r) * C + u] = logit[r][u];
      }
    }
    __syncthreads();
    if (wave < nr) {
      const int r = wave;
      float v[DEC_CMAX / 64];
      float m = -INFINITY;
#pragma unroll
      for (int i = 0; i < DEC_CMAX / 64; ++i) {
        const int cidx = lane + 64 * i;
        v[i] = cidx < C ? logit[r][cidx] : -INFINITY;
        m = fmaxf(m, v[i]);
      }
      m = wave_max(m);
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DEC_CMAX / 64; ++i) { v[i] = (lane + 64 * i) < C ? expf(v[i] - m) : 0.f; s += v[i]; }
      s = wave_sum(s);
      float best = -1.f;
      int besti = 0x7fffffff;
      float* o = p.out + ((long)(r0 + r) * p.max_len + step) * C;
#pragma unroll
      for (int i = 0; i < DEC_CMAX / 64; ++i) {
        const int cidx = lane + 64 * i;
        if (cidx < C) {
          const float pr = v[i] / s;
          o[cidx] = pr;
          if (pr > best) { best = pr; besti = cidx; }
        }
      }
      wave_argmax_first(best, besti);
      if (lane == 0) {
        // a NaN or +inf logit makes every probability NaN, no lane offers an index and besti is still the sentinel: the
        // symbol indexes the embedding table below and in the next step, so it is bound to [0, C) (the sentinel becomes
        // C - 1, the symbol the persistent kernel feeds); a finite row's arg-max is in range and passes unchanged
        const int y = min(max(besti, 0), C - 1);
        ycur[r] = y;
        p.yprev[r0 + r] = y;
        p.pred[(long)(r0 + r) * p.max_len + step] = y;
      }
    }
    __syncthreads();
  }
  if (!do_att) return;
  // ---- sProj = sEmbed(h)
  {
    float acc[1][DEC_RB];
#pragma unroll
    for (int r = 0; r < DEC_RB; ++r) acc[0][r] = p.sB[u];
    stream_matvec<1, DEC_RB, 16>(reinterpret_cast<const float4*>(p.sW), DEC_D, 0, u, DEC_D / 4, &h[0][0], DEC_D, acc);
#pragma unroll
    for (int r = 0; r < DEC_RB; ++r) sproj[r][u] = acc[0][r];
  }
  __syncthreads();
  // ---- energies e[r][t] = wEmbed(tanh(sProj + xProj[t])): wavefront per (r,t), lanes over D
  {
    const float4 ww = *reinterpret_cast<const float4*>(p.wW + lane * 4);
    const float wb = p.wB[0];
    const int npairs = nr * T;
    for (int base = wave; base < npairs; base += 4 * 8) {
      float4 xp[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pr = min(base + 4 * i, npairs - 1);
        const int r = pr / T, t = pr - r * T;
        xp[i] = *reinterpret_cast<const float4*>(p.xproj + ((long)(r0 + r) * T + t) * DEC_D + lane * 4);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pr = base + 4 * i;
        if (pr < npairs) {
          const int r = pr / T, t = pr - r * T;
          const float4 sp = *reinterpret_cast<const float4*>(&sproj[r][lane * 4]);
          float s = ww.x * tanh_fast(sp.x + xp[i].x) + ww.y * tanh_fast(sp.y + xp[i].y) + ww.z * tanh_fast(sp.z + xp[i].z) +
                    ww.w * tanh_fast(sp.w + xp[i].w);
          s = wave_sum(s);
          if (lane == 0) energy[r][t] = s + wb;
        }
      }
    }
  }
  __syncthreads();
  if (wave < nr) {
    const int r = wave;
    const float v = lane < T ? energy[r][lane] : -INFINITY;
    const float m = wave_max(v);
    const float e = lane < T ? expf(v - m) : 0.f;
    const float s = wave_sum(e);
    if (lane < T) energy[r][lane] = e / s;
  }
  __syncthreads();
  // ---- inp = [embedding(y) | context = alpha . x]
  for (int r = 0; r < nr; ++r) {
    float s = 0.f;
    const float* xr = p.x + (long)(r0 + r) * T * DEC_D + u;
    int t = 0;
    for (; t + 16 <= T; t += 16) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = xr[(long)(t + i) * DEC_D];
#pragma unroll
      for (int i = 0; i < 16; ++i) s += energy[r][t + i] * v[i];
    }
    for (; t < T; ++t) s += energy[r][t] * xr[(long)t * DEC_D];
    float* ip = p.inp + (long)(r0 + r) * (2 * DEC_D);
    ip[u] = p.emb[(long)ycur[r] * DEC_D + u];
    ip[DEC_D + u] = s;
  }
}

// h_next = GRUCell(inp, h_prev): grid (ceil(R/16), D/GRU_UB).  The workgroup's 3*GRU_UB gate rows (3 gates x GRU_UB
// units) are 3*GRU_UB/16 row tiles of 16; each tile has three K-slices of 256 (W_ih[:, :256], W_ih[:, 256:], W_hh):
// 9*GRU_UB/16 MFMA jobs of 64 MFMAs, dealt round-robin to the 4 wavefronts; slices are summed in the pointwise phase.
__global__ __launch_bounds__(256) void dec_gru_kernel(DecParams p, const float* __restrict__ hprev, float* __restrict__ hnext) {
  __shared__ __attribute__((aligned(16))) float xin[GRU_RB][2 * DEC_D + 4];
  __shared__ __attribute__((aligned(16))) float hs[GRU_RB][DEC_D + 4];
  __shared__ float gbuf[3][GRU_RB][3 * GRU_UB + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * GRU_RB, ub = blockIdx.y;
  const int nr = min(GRU_RB, p.R - r0);
  for (int i = tid; i < GRU_RB * (2 * DEC_D / 4); i += 256) {
    const int r = i / (2 * DEC_D / 4), k4 = i % (2 * DEC_D / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nr) v = reinterpret_cast<const float4*>(p.inp + (long)(r0 + r) * (2 * DEC_D))[k4];
    *reinterpret_cast<float4*>(&xin[r][k4 * 4]) = v;
  }
  for (int i = tid; i < GRU_RB * (DEC_D / 4); i += 256) {
    const int r = i / (DEC_D / 4), k4 = i % (DEC_D / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nr) v = reinterpret_cast<const float4*>(hprev + (long)(r0 + r) * DEC_D)[k4];
    *reinterpret_cast<float4*>(&hs[r][k4 * 4]) = v;
  }
  __syncthreads();
  constexpr int NT = GRU_UB / 16;                           // 16-row MFMA tiles per gate
  for (int job = wave; job < 9 * NT; job += 4) {
    const int tile = job / 3, part = job - tile * 3;        // part 0/1: W_ih column halves, 2: W_hh
    const int g = tile / NT, uh = tile - g * NT;
    const int row0 = g * DEC_D + ub * GRU_UB + uh * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (part < 2) mfma_rows16<DEC_D>(p.w_ih + part * DEC_D, 2 * DEC_D, row0, &xin[0][part * DEC_D], 2 * DEC_D + 4, lane, acc);
    else mfma_rows16<DEC_D>(p.w_hh, DEC_D, row0, &hs[0][0], DEC_D + 4, lane, acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) gbuf[part][lane & 15][g * GRU_UB + uh * 16 + (lane >> 4) * 4 + e] = acc[e];
  }
  __syncthreads();
  for (int i = tid; i < GRU_RB * GRU_UB; i += 256) {
    const int r = i / GRU_UB, ul = i % GRU_UB;
    if (r < nr) {
      const int u = ub * GRU_UB + ul;
      const float ir = gbuf[0][r][ul] + gbuf[1][r][ul] + p.b_ih[u];
      const float iz = gbuf[0][r][GRU_UB + ul] + gbuf[1][r][GRU_UB + ul] + p.b_ih[DEC_D + u];
      const float in_ = gbuf[0][r][2 * GRU_UB + ul] + gbuf[1][r][2 * GRU_UB + ul] + p.b_ih[2 * DEC_D + u];
      const float hr = gbuf[2][r][ul] + p.b_hh[u];
      const float hz = gbuf[2][r][GRU_UB + ul] + p.b_hh[DEC_D + u];
      const float hn = gbuf[2][r][2 * GRU_UB + ul] + p.b_hh[2 * DEC_D + u];
      const float rg = sigmoidf_(ir + hr), zg = sigmoidf_(iz + hz);
      const float ng = tanhf(in_ + rg * hn);
      hnext[(long)(r0 + r) * DEC_D + u] = (1.f - zg) * ng + zg * hs[r][u];
    }
  }
}

void dec_gru_step(const DecParams& p, const float* hprev, float* hnext, hipStream_t stream) {
  hipLaunchKernelGGL(dec_gru_kernel, dim3(cdiv(p.R, GRU_RB), DEC_D / GRU_UB), dim3(256), 0, stream, p, hprev, hnext);
}

// one launch of dec_fc_att_kernel on the p.R rows, blocked by the row count (see DEC_RB)
static void dec_fc_att_step(const DecParams& p, const float* hcur, int step, int do_att, hipStream_t stream) {
  const int rb = p.R >= 1024 ? 4 : p.R >= 512 ? 2 : 1;
  const dim3 ga(cdiv(p.R, rb));
  if (rb == 4) hipLaunchKernelGGL(dec_fc_att_kernel<4>, ga, dim3(256), 0, stream, p, hcur, step, do_att);
  else if (rb == 2) hipLaunchKernelGGL(dec_fc_att_kernel<2>, ga, dim3(256), 0, stream, p, hcur, step, do_att);
  else hipLaunchKernelGGL(dec_fc_att_kernel<1>, ga, dim3(256), 0, stream, p, hcur, step, do_att);
}

DecParams dec_params(const float* x, const float* xproj, const glass_decoder_weights* w, int rows, int T, int C, int max_len) {
  DecParams p;
  p.x = x; p.xproj = xproj; p.sW = w->sW; p.sB = w->sB; p.wW = w->wW; p.wB = w->wB; p.emb = w->emb; p.w_ih = w->w_ih;
  p.w_hh = w->w_hh; p.b_ih = w->b_ih; p.b_hh = w->b_hh; p.fcW = w->fcW; p.fcB = w->fcB; p.temperature = w->temperature;
  p.R = rows; p.T = T; p.C = C; p.max_len = max_len;
  p.out = nullptr; p.pred = nullptr; p.h0 = p.h1 = p.inp = nullptr; p.yprev = nullptr; p.logits = nullptr;
  return p;
}

extern "C" int64_t glass_decode_workspace_bytes(int R, int D) {
  return (int64_t)((size_t)R * D * 2 + (size_t)R * 2 * D) * sizeof(float) + (int64_t)R * sizeof(int);
}

extern "C" int glass_attention_decode(const float* x, const float* xproj, const glass_decoder_weights* w, const int* roi_image,
                                      int R, int num_images, int T, int D, int C, int max_len, int eos, float* out,
                                      int* pred_scratch, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(D == DEC_D && T > 0 && T <= DEC_TMAX && C > 0 && C <= DEC_CMAX && max_len > 0,
                  "glass_attention_decode: needs D=256, T<=64, C<=256 (got D=%d T=%d C=%d)", D, T, C);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(x && xproj && w && roi_image && out && pred_scratch && num_images > 0 && workspace,
                  "glass_attention_decode: null pointer");
  GLASS_CHECK_ARG(workspace_bytes >= glass_decode_workspace_bytes(R, D), "glass_attention_decode: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  DecParams p = dec_params(x, xproj, w, R, T, C, max_len);
  p.out = out; p.pred = pred_scratch;
  float* ws = static_cast<float*>(workspace);
  p.h0 = ws; p.h1 = ws + (size_t)R * D; p.inp = ws + (size_t)R * D * 2;
  p.yprev = reinterpret_cast<int*>(ws + (size_t)R * D * 4);
  hipError_t e = hipMemsetAsync(p.h0, 0, (size_t)R * D * sizeof(float), s);      // initial state h = 0
  if (e != hipSuccess) { glass_set_error("glass_attention_decode: memset: %s", hipGetErrorString(e)); return GLASS_EHIP; }
  float* hb[2] = {p.h0, p.h1};
  dec_fc_att_step(p, hb[0], -1, 1, s);                                                        // attention for step 0
  for (int step = 0; step < max_len; ++step) {
    dec_gru_step(p, hb[step & 1], hb[(step + 1) & 1], s);
    dec_fc_att_step(p, hb[(step + 1) & 1], step, step + 1 < max_len ? 1 : 0, s);
  }
  GLASS_CHECK_LAUNCH("glass_attention_decode");
  hipLaunchKernelGGL(decode_break_mask_kernel, dim3(num_images), dim3(256), 0, s, pred_scratch, roi_image, R, max_len, C, eos,
                     out);
  GLASS_CHECK_LAUNCH("glass_attention_decode(mask)");
  return GLASS_OK;
}

// One decoder step for a caller-driven search (AttentionRecognitionHead.beam_search, reference prediction_aster.py:133-134:
// `output, state, alpha = self.decoder(x, state, y_prev)`): attention with h_in and the embedding of y_prev, GRU cell, fc.
extern "C" int64_t glass_decode_step_workspace_bytes(int R, int D) {
  return (int64_t)((size_t)R * 2 * D) * sizeof(float) + (int64_t)R * 2 * sizeof(int);
}

extern "C" int glass_attention_decode_step(const float* x, const float* xproj, const glass_decoder_weights* w, int R, int T, int D,
                                           int C, const float* h_in, const int* y_prev, float* h_out, float* logits_out,
                                           float* probs_out, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(D == DEC_D && T > 0 && T <= DEC_TMAX && C > 0 && C <= DEC_CMAX,
                  "glass_attention_decode_step: needs D=256, T<=64, C<=256 (got D=%d T=%d C=%d)", D, T, C);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(x && xproj && w && h_in && y_prev && h_out && logits_out && probs_out && workspace && h_in != h_out,
                  "glass_attention_decode_step: null pointer (or h_out aliases h_in)");
  GLASS_CHECK_ARG(workspace_bytes >= glass_decode_step_workspace_bytes(R, D), "glass_attention_decode_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  DecParams p = dec_params(x, xproj, w, R, T, C, 1);
  p.out = probs_out;
  float* ws = static_cast<float*>(workspace);
  p.inp = ws;
  int* iscratch = reinterpret_cast<int*>(ws + (size_t)R * 2 * D);
  p.pred = iscratch;
  p.yprev = const_cast<int*>(y_prev);            // read only in the attention-only launch
  dec_fc_att_step(p, h_in, -2, 1, s);            // inp = [embedding(y_prev) | attention context of h_in]
  dec_gru_step(p, h_in, h_out, s);
  p.yprev = iscratch + R;                        // the fc launch records its arg-max: into the scratch, not into the caller's y
  p.logits = logits_out;
  dec_fc_att_step(p, h_out, 0, 0, s);            // logits = fc(h_out) * temperature, probs = softmax(logits)
  GLASS_CHECK_LAUNCH("glass_attention_decode_step");
  return GLASS_OK;
}

