// Global-to-local fusion attention of the per-RoI recognition head (softmax pooling + channel MLP), independent across RoIs.
// Reductions (softmax, LayerNorm, mask logits) are wavefront DPP reductions (64 lanes) + one LDS hop across the 4 wavefronts.
#include "recognition_common.h"

// one workgroup (256 threads) per RoI; x slab [HW=256][C=512]
constexpr int GC_C = 512, GC_HW = 256, GC_HEADS = 8, GC_P = 256;

__global__ __launch_bounds__(256) void gc_attention_kernel(float* __restrict__ xall, const float* __restrict__ w_mask,
                                                           const float* __restrict__ b_mask, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ ln_g,
                                                           const float* __restrict__ ln_b, const float* __restrict__ w2,
                                                           const float* __restrict__ b2) {
  __shared__ float prob[GC_HEADS][GC_HW];   // mask logits, then softmax probabilities
  __shared__ float ctx[GC_C];
  __shared__ float hid[GC_P];
  __shared__ float red[8];
  float* x = xall + (long)blockIdx.x * GC_HW * GC_C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // phase 1: mask logits. A wavefront covers one position per iteration: lane l holds channels
  // 4l..4l+3 and 256+4l..; a head is 64 channels = 16 lanes -> 4-step shuffle reduction.
  // (8 positions = 16 independent 16-byte loads per lane in flight per trip: the slab streams from HBM, and one position per
  //  trip - the shuffles and the LDS store keep the compiler from overlapping trips - made this phase 64 serial round trips)
  const float4 wm = *reinterpret_cast<const float4*>(w_mask + ((lane * 4) & 63));
  const float bm = b_mask[0];
  constexpr int GC_U1 = 8;
  static_assert(GC_HW % (4 * GC_U1) == 0, "phase 1 unroll");
  for (int pos0 = wave; pos0 < GC_HW; pos0 += 4 * GC_U1) {
    float4 a[GC_U1], b[GC_U1];
#pragma unroll
    for (int i = 0; i < GC_U1; ++i) {
      a[i] = *reinterpret_cast<const float4*>(x + (long)(pos0 + 4 * i) * GC_C + lane * 4);
      b[i] = *reinterpret_cast<const float4*>(x + (long)(pos0 + 4 * i) * GC_C + 256 + lane * 4);
    }
#pragma unroll
    for (int i = 0; i < GC_U1; ++i) {
      float sa = a[i].x * wm.x + a[i].y * wm.y + a[i].z * wm.z + a[i].w * wm.w;
      float sb = b[i].x * wm.x + b[i].y * wm.y + b[i].z * wm.z + b[i].w * wm.w;
      sa = row16_sum(sa);
      sb = row16_sum(sb);
      if ((lane & 15) == 0) {
        prob[lane >> 4][pos0 + 4 * i] = sa + bm;
        prob[4 + (lane >> 4)][pos0 + 4 * i] = sb + bm;
      }
    }
  }
  __syncthreads();
  // phase 2: softmax over the 256 positions of each head (2 heads per wavefront)
  for (int h = wave * 2; h < wave * 2 + 2; ++h) {
    float v[4], m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = prob[h][lane + 64 * i]; m = fmaxf(m, v[i]); }
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = expf(v[i] - m); s += v[i]; }
    s = wave_sum(s);
#pragma unroll
    for (int i = 0; i < 4; ++i) prob[h][lane + 64 * i] = v[i] / s;
  }
  __syncthreads();
  // phase 3: context[c] = sum_pos x[pos][c] * prob[head(c)][pos]; thread owns channels tid, tid+256
  {
    float c0 = 0.f, c1 = 0.f;
    const int h0 = tid >> 6, h1 = 4 + (tid >> 6);
    constexpr int GC_U3 = 16;                                   // 32 independent loads per thread in flight
    for (int pos0 = 0; pos0 < GC_HW; pos0 += GC_U3) {
      float v0[GC_U3], v1[GC_U3];
#pragma unroll
      for (int i = 0; i < GC_U3; ++i) {
        v0[i] = x[(long)(pos0 + i) * GC_C + tid];
        v1[i] = x[(long)(pos0 + i) * GC_C + 256 + tid];
      }
      // the 16 products of a trip are summed as a tree and join the running sum once: 256 dependent additions drift when the
      // terms are alike (a head with a uniform softmax sums 256 x v/256: 6e-6 on the output, six times the error of a plain
      // fp32 evaluation - tests/test_gpu_recognition_edges.py), 16 additions of 16-term trees do not
#pragma unroll
      for (int i = 0; i < GC_U3; i += 2) {
        v0[i] = __fmaf_rn(v0[i + 1], prob[h0][pos0 + i + 1], v0[i] * prob[h0][pos0 + i]);
        v1[i] = __fmaf_rn(v1[i + 1], prob[h1][pos0 + i + 1], v1[i] * prob[h1][pos0 + i]);
      }
#pragma unroll
      for (int s = 2; s < GC_U3; s *= 2) {
#pragma unroll
        for (int i = 0; i < GC_U3; i += 2 * s) {
          v0[i] += v0[i + s];
          v1[i] += v1[i + s];
        }
      }
      c0 += v0[0];
      c1 += v1[0];
    }
    ctx[tid] = c0;
    ctx[256 + tid] = c1;
  }
  __syncthreads();
  // phase 4a: hid = W1 ctx + b1 (256 x 512): each wavefront takes rows wave, wave+4, ...
  // (8 rows per trip: the weight rows come from L2 and the reduction after each row kept one row in flight - 64 serial L2
  //  round trips per wavefront here, 128 in phase 4b)
  {
    constexpr int GC_U4 = 8;
    static_assert(GC_P % (4 * GC_U4) == 0 && GC_C % (4 * GC_U4) == 0, "phase 4 unroll");
    const float4 ca = *reinterpret_cast<const float4*>(ctx + lane * 4);
    const float4 cb = *reinterpret_cast<const float4*>(ctx + 256 + lane * 4);
    for (int j0 = wave; j0 < GC_P; j0 += 4 * GC_U4) {
      float4 wa[GC_U4], wb[GC_U4];
#pragma unroll
      for (int i = 0; i < GC_U4; ++i) {
        wa[i] = *reinterpret_cast<const float4*>(w1 + (long)(j0 + 4 * i) * GC_C + lane * 4);
        wb[i] = *reinterpret_cast<const float4*>(w1 + (long)(j0 + 4 * i) * GC_C + 256 + lane * 4);
      }
#pragma unroll
      for (int i = 0; i < GC_U4; ++i) {
        float s = wa[i].x * ca.x + wa[i].y * ca.y + wa[i].z * ca.z + wa[i].w * ca.w + wb[i].x * cb.x + wb[i].y * cb.y + wb[i].z * cb.z +
                  wb[i].w * cb.w;
        s = wave_sum(s);
        if (lane == 0) hid[j0 + 4 * i] = s + b1[j0 + 4 * i];
      }
    }
  }
  __syncthreads();
  // LayerNorm over the 256 hidden values (biased variance, eps 1e-5) + ReLU
  {
    const float v = hid[tid];
    float s = wave_sum(v);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)GC_P;
    const float d = v - mean;
    float q = wave_sum(d * d);
    if (lane == 0) red[4 + wave] = q;
    __syncthreads();
    const float var = (red[4] + red[5] + red[6] + red[7]) / (float)GC_P;
    const float y = d / sqrtf(var + 1e-5f) * ln_g[tid] + ln_b[tid];
    __syncthreads();
    hid[tid] = fmaxf(y, 0.f);
  }
  __syncthreads();
  // phase 4b: t = W2 hid + b2 (512 x 256) -> reuse ctx[] for t
  {
    constexpr int GC_U4 = 8;
    const float4 hv = *reinterpret_cast<const float4*>(hid + lane * 4);
    for (int c0 = wave; c0 < GC_C; c0 += 4 * GC_U4) {
      float4 wv[GC_U4];
#pragma unroll
      for (int i = 0; i < GC_U4; ++i) wv[i] = *reinterpret_cast<const float4*>(w2 + (long)(c0 + 4 * i) * GC_P + lane * 4);
#pragma unroll
      for (int i = 0; i < GC_U4; ++i) {
        float s = wv[i].x * hv.x + wv[i].y * hv.y + wv[i].z * hv.z + wv[i].w * hv.w;
        s = wave_sum(s);
        if (lane == 0) ctx[c0 + 4 * i] = s + b2[c0 + 4 * i];
      }
    }
  }
  __syncthreads();
  // phase 5: x += t (broadcast over positions), float4 streaming
  {
    const int c4 = tid & 127;           // 128 float4 per position
    const float4 t = *reinterpret_cast<const float4*>(ctx + c4 * 4);
    constexpr int GC_U5 = 16;
    for (int pos0 = tid >> 7; pos0 < GC_HW; pos0 += 2 * GC_U5) {
      float4 v[GC_U5];
#pragma unroll
      for (int i = 0; i < GC_U5; ++i) v[i] = *(reinterpret_cast<const float4*>(x + (long)(pos0 + 2 * i) * GC_C) + c4);
#pragma unroll
      for (int i = 0; i < GC_U5; ++i) {
        v[i].x += t.x; v[i].y += t.y; v[i].z += t.z; v[i].w += t.w;
        *(reinterpret_cast<float4*>(x + (long)(pos0 + 2 * i) * GC_C) + c4) = v[i];
      }
    }
  }
}

extern "C" int glass_gc_attention_inplace(float* x, int R, int HW, int C, int heads, int P, const float* w_mask,
                                          const float* b_mask, const float* w1, const float* b1, const float* ln_g,
                                          const float* ln_b, const float* w2, const float* b2, glass_stream_t stream) {
  GLASS_CHECK_ARG(C == GC_C && HW == GC_HW && heads == GC_HEADS && P == GC_P,
                  "glass_gc_attention_inplace: only C=512, HW=256, heads=8, P=256 is built (got %d,%d,%d,%d)", C, HW, heads, P);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(x && w_mask && b_mask && w1 && b1 && ln_g && ln_b && w2 && b2, "glass_gc_attention_inplace: null pointer");
  hipLaunchKernelGGL(gc_attention_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, x, w_mask, b_mask, w1, b1, ln_g, ln_b,
                     w2, b2);
  GLASS_CHECK_LAUNCH("glass_gc_attention_inplace");
  return GLASS_OK;
}
