// Where inside its box every character of a word lies (include/glass_hip_feature_chars.h states the contract;
// glass_amd/postprocess/char_boxes.py::char_spans_host is the statement of the spans in numpy float64):
//   glass_char_spans: the attention rows of a forced replay [R][L][T] -> normalised spans along the box's width, one wavefront
//                     per word, a lane per encoder column, the steps in a loop, the word's centres in LDS for the boundaries
//   glass_char_quads: spans + the pooled box -> the four corners of every character in the image, a thread per (word, step)
// Every value is widened exactly to float64, every formula is evaluated in float64 without contraction and rounded to float32
// once.  Nothing read from memory is used as an index: a length is clamped to [0, L], a symbol is only compared with eos.
#include "common.h"
#include "glass_hip_feature_chars.h"

#pragma clang fp contract(off)

constexpr int CB_LMAX = 64;   // steps of a word (BEAM_LMAX of the decoder searches)
constexpr int CB_TMAX = 64;   // encoder columns (DEC_TMAX): one lane each

// the sum over the 64 lanes by a fixed butterfly: the same bits in every lane and from run to run
__device__ __forceinline__ double cb_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double cb_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

__global__ __launch_bounds__(64) void cb_spans_kernel(const float* __restrict__ att, const int* __restrict__ targets,
                                                      const int* __restrict__ lengths, int L, int T, int eos,
                                                      float* __restrict__ spans, float* __restrict__ centres,
                                                      float* __restrict__ spreads, int* __restrict__ count,
                                                      int* __restrict__ monotone, int* __restrict__ valid) {
  __shared__ double cen[CB_LMAX], spr[CB_LMAX];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int len = min(max(lengths[r], 0), L);
  int m = len;
  if (len > 0 && targets[(long)r * L + len - 1] == eos) m = len - 1;
  const double p = ((double)lane + 0.5) / (double)T;
  const float* rows = att + (long)r * L * T;
  bool ok = true;                                                // uniform over the wavefront
  for (int t = 0; t < m; ++t) {
    const double a = lane < T ? (double)rows[(long)t * T + lane] : 0.0;
    const bool bad = !(a >= 0.0 && a < (double)INFINITY);         // a NaN fails the first comparison
    const double S = cb_wave_sum(a);
    const double c = cb_wave_sum(a * p) / S;
    const double d = p - c;
    const double s = sqrt(cb_wave_sum(a * (d * d)) / S);
    if (__any(bad) || !(S > 0.0 && S < (double)INFINITY)) ok = false;
    if (lane == 0) { cen[t] = c; spr[t] = s; }
  }
  __syncthreads();
  if (!ok) m = 0;
  const bool falls = lane + 1 < m && !(cen[lane + 1] > cen[lane]);
  const int mono = __any(falls) ? 0 : 1;
  if (lane == 0) { count[r] = m; monotone[r] = ok ? mono : 0; valid[r] = ok ? 1 : 0; }
  if (lane < L) {
    const int t = lane;
    double lo = 0.0, hi = 0.0, c = 0.0, s = 0.0;
    if (t < m) {
      c = cen[t];
      s = spr[t];
      if (m == 1) { lo = 0.0; hi = 1.0; }
      else {
        double l, rr;
        if (t == 0) { const double b0 = (cen[0] + cen[1]) / 2.0; l = cb_clamp01(cen[0] - fabs(b0 - cen[0])); }
        else l = (cen[t - 1] + cen[t]) / 2.0;
        if (t == m - 1) { const double bl = (cen[m - 2] + cen[m - 1]) / 2.0; rr = cb_clamp01(cen[m - 1] + fabs(cen[m - 1] - bl)); }
        else rr = (cen[t] + cen[t + 1]) / 2.0;
        lo = fmin(l, rr);
        hi = fmax(l, rr);
      }
    }
    const long o = (long)r * L + t;
    spans[o * 2] = (float)lo;
    spans[o * 2 + 1] = (float)hi;
    centres[o] = (float)c;
    spreads[o] = (float)s;
  }
}

__global__ __launch_bounds__(256) void cb_quads_kernel(const float* __restrict__ spans, const int* __restrict__ count,
                                                       const float* __restrict__ frames, long n, int L, float* __restrict__ quads) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long r = i / L;
  const int t = (int)(i - r * L);
  const int m = min(max(count[r], 0), L);
  const float* f = frames + r * 5;
  const double cx = f[0], cy = f[1], w = f[2], h = f[3], ang = f[4];
  const double big = (double)INFINITY;
  const bool frame_ok = fabs(cx) < big && fabs(cy) < big && w > 0.0 && w < big && h > 0.0 && h < big && fabs(ang) < big;
  double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (t < m && frame_ok) {
    const double lo = spans[i * 2], hi = spans[i * 2 + 1];
    const double th = ang * 3.14159265358979323846 / 180.0;
    const double ct = cos(th), st = sin(th);
    const double ux = ct, uy = -st, vx = st, vy = ct;            // width along u, height along v (csrc/roi_align.hip)
    const double off = ((lo + hi) / 2.0 - 0.5) * w;
    const double mx = cx + off * ux, my = cy + off * uy;
    const double e = (hi - lo) * w / 2.0, g = h / 2.0;
    q[0] = mx - e * ux - g * vx; q[1] = my - e * uy - g * vy;
    q[2] = mx + e * ux - g * vx; q[3] = my + e * uy - g * vy;
    q[4] = mx + e * ux + g * vx; q[5] = my + e * uy + g * vy;
    q[6] = mx - e * ux + g * vx; q[7] = my - e * uy + g * vy;
  }
  float* o = quads + i * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (float)q[k];
}

extern "C" int glass_char_spans(const float* attention, const int* targets, const int* lengths, int R, int L, int T, int eos,
                                float* spans, float* centres, float* spreads, int* count, int* monotone, int* valid,
                                glass_stream_t stream) {
  GLASS_CHECK_ARG(R >= 0 && L >= 1 && L <= CB_LMAX && T >= 1 && T <= CB_TMAX,
                  "glass_char_spans: needs R>=0, 1<=L<=64, 1<=T<=64 (got R=%d L=%d T=%d)", R, L, T);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(attention && targets && lengths && spans && centres && spreads && count && monotone && valid,
                  "glass_char_spans: null pointer");
  hipLaunchKernelGGL(cb_spans_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, attention, targets, lengths, L, T, eos, spans,
                     centres, spreads, count, monotone, valid);
  GLASS_CHECK_LAUNCH("glass_char_spans");
  return GLASS_OK;
}

extern "C" int glass_char_quads(const float* spans, const int* count, const float* frames, int R, int L, float* quads,
                                glass_stream_t stream) {
  GLASS_CHECK_ARG(R >= 0 && L >= 1 && L <= CB_LMAX, "glass_char_quads: needs R>=0, 1<=L<=64 (got R=%d L=%d)", R, L);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(spans && count && frames && quads, "glass_char_quads: null pointer");
  const long n = (long)R * L;
  hipLaunchKernelGGL(cb_quads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, spans, count, frames,
                     n, L, quads);
  GLASS_CHECK_LAUNCH("glass_char_quads");
  return GLASS_OK;
}
