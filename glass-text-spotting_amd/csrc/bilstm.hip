// BiLSTM recurrence of the per-RoI recognition head, independent across RoIs: ONE LAUNCH PER DEPENDENT STEP, all issued by a
// single ABI call with no host synchronisation (state double-buffered in a global workspace, previous rows staged in LDS).
// The step runs on 16x16x4 fp32 MFMA tiles (8 us per step; a persistent workgroup per RoI group took 27 us: DESIGN.md section 3).
#include "recognition_common.h"

// One launch per time step (T launches per layer, issued back to back by the host function).  A persistent
// workgroup per RoI group would have to stream the whole 1 MiB recurrent matrix through ONE CU every step
// (~40 GB/s per CU -> 27 us/step); instead each step is spread over the chip: grid = (RoI groups of 16,
// 8 blocks of 32 hidden units, 2 directions), every workgroup streams only its 128 KiB weight slice
// (4 gates x 32 units x 256) from L2 and keeps the 16 previous hidden rows in LDS.  The hidden/cell state
// lives in a small global workspace, double-buffered across launches (stream order is the barrier).
constexpr int LSTM_HD = 256;
constexpr int LS_RB = 16;   // RoIs per workgroup (= the N of a 16x16x4 MFMA)
constexpr int LS_UB = 32;   // hidden units per workgroup

__global__ __launch_bounds__(256) void lstm_step_kernel(const float* __restrict__ xg, const float* __restrict__ whh,
                                                        const float* __restrict__ h_prev, float* __restrict__ h_next,
                                                        float* __restrict__ c_state, float* __restrict__ out, int R, int T,
                                                        int step) {
  __shared__ __attribute__((aligned(16))) float hs[LS_RB][LSTM_HD + 4];   // +4: 16-byte row skew against bank conflicts
  __shared__ float gates[LS_RB][4 * LS_UB + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = blockIdx.z, ub = blockIdx.y, r0 = blockIdx.x * LS_RB;
  const int t = dir == 0 ? step : T - 1 - step;
  const int nr = min(LS_RB, R - r0);
  for (int i = tid; i < LS_RB * (LSTM_HD / 4); i += 256) {
    const int r = i / (LSTM_HD / 4), k4 = i % (LSTM_HD / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < nr) v = reinterpret_cast<const float4*>(h_prev + ((long)(r0 + r) * 2 + dir) * LSTM_HD)[k4];
    *reinterpret_cast<float4*>(&hs[r][k4 * 4]) = v;
  }
  __syncthreads();
  // the workgroup's 128 gate rows = 8 row tiles of 16: tile = gate * 2 + half-of-32-units; 2 tiles per wavefront
  const float* W = whh + (long)dir * (4 * LSTM_HD) * LSTM_HD;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int tile = wave * 2 + q;
    const int g = tile >> 1, uh = tile & 1;
    const int row0 = g * LSTM_HD + ub * LS_UB + uh * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    mfma_rows16<LSTM_HD>(W, LSTM_HD, row0, &hs[0][0], LSTM_HD + 4, lane, acc);
    // C layout: col = lane & 15 (RoI), row = (lane >> 4) * 4 + e
#pragma unroll
    for (int e = 0; e < 4; ++e) gates[lane & 15][g * LS_UB + uh * 16 + (lane >> 4) * 4 + e] = acc[e];
  }
  __syncthreads();
  for (int i = tid; i < LS_RB * LS_UB; i += 256) {
    const int r = i / LS_UB, ul = i % LS_UB;
    if (r < nr) {
      const int u = ub * LS_UB + ul;
      const long idx = ((long)(r0 + r) * 2 + dir) * LSTM_HD + u;
      const float* xr = xg + (((long)(r0 + r) * T + t) * 2 + dir) * (4 * LSTM_HD) + u;
      const LstmCell cell = lstm_cell(xr[0] + gates[r][ul], xr[LSTM_HD] + gates[r][LS_UB + ul], xr[2 * LSTM_HD] + gates[r][2 * LS_UB + ul],
                                      xr[3 * LSTM_HD] + gates[r][3 * LS_UB + ul], c_state[idx]);
      c_state[idx] = cell.c;
      const float hn = cell.h;
      h_next[idx] = hn;
      out[((long)(r0 + r) * T + t) * (2 * LSTM_HD) + dir * LSTM_HD + u] = hn;
    }
  }
}

extern "C" int64_t glass_bilstm_workspace_bytes(int R, int Hd) { return (int64_t)3 * R * 2 * Hd * sizeof(float); }

extern "C" int glass_bilstm_recurrence(const float* xg, const float* w_hh_packed, float* out, int R, int T, int Hd,
                                       void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(Hd == LSTM_HD, "glass_bilstm_recurrence: only Hd=256 is built (got %d)", Hd);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(xg && w_hh_packed && out && T > 0 && workspace, "glass_bilstm_recurrence: bad args");
  GLASS_CHECK_ARG(workspace_bytes >= glass_bilstm_workspace_bytes(R, Hd), "glass_bilstm_recurrence: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)R * 2 * Hd;
  float* hbuf[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + n};
  float* c = static_cast<float*>(workspace) + 2 * n;
  hipError_t e = hipMemsetAsync(workspace, 0, 3 * n * sizeof(float), s);     // h0 = c0 = 0
  if (e != hipSuccess) { glass_set_error("glass_bilstm_recurrence: memset: %s", hipGetErrorString(e)); return GLASS_EHIP; }
  const dim3 grid(cdiv(R, LS_RB), LSTM_HD / LS_UB, 2);
  for (int step = 0; step < T; ++step)
    hipLaunchKernelGGL(lstm_step_kernel, grid, dim3(256), 0, s, xg, w_hh_packed, hbuf[step & 1], hbuf[(step + 1) & 1], c, out,
                       R, T, step);
  GLASS_CHECK_LAUNCH("glass_bilstm_recurrence");
  return GLASS_OK;
}
