// Rotated mask branch at inference: the pieces around the conv stack that are not convolutions.
//   * 2x pixel shuffle that turns the 1x1-conv form of ConvTranspose2d(k=2, s=2) into the 28x28 map,
//   * sigmoid (d2 mask_rcnn_inference),
//   * rotated mask paste = the reference's own paste_masks_in_image / _do_paste_mask
//     (glass/postprocess/post_processor_academic.py:187-335): per RoI a sampling grid centred on the box,
//     rotated by its angle, normalised to the box, bilinear grid_sample (align_corners=False, zero padding)
//     of the MxM mask over the whole image, threshold.
#include "common.h"
#include "mask_paste_common.h"
#include <cstdint>

namespace {

static inline int grid_for_n(long n, int block) {
  long g = (n + block - 1) / block;
  if (g > 256L * 32) g = 256L * 32;
  if (g < 1) g = 1;
  return (int)g;
}

// x [N,H,W,4*C] with channel = (a*2+b)*C + c  ->  y [N,2H,2W,C],  y[n,2h+a,2w+b,c] = x[n,h,w,(a*2+b)*C+c]
__global__ void pixel_shuffle2x_kernel(const float4* __restrict__ x, float4* __restrict__ y, int N, int H, int W, int C4) {
  const long total = (long)N * H * W * 4 * C4;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(idx % C4);
    long t = idx / C4;
    const int ab = (int)(t & 3);
    t >>= 2;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H);
    const int n = (int)(t / H);
    const int a = ab >> 1, b = ab & 1;
    y[(((long)n * 2 * H + 2 * h + a) * 2 * W + 2 * w + b) * C4 + c4] = x[idx];
  }
}

__global__ void sigmoid_kernel(float* __restrict__ x, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = 1.f / (1.f + expf(-x[i]));
}

struct PasteParams {
  const float* masks;   // [R,M,M]
  const float* boxes;   // [R,5]
  uint8_t* out;         // [R,H,W]
  int R, M, H, W;
  float threshold;
};

// one thread per 4 consecutive output pixels of one RoI row (32-bit packed store).  The per-pixel arithmetic, bit-exact
// against the reference's torch-CPU path, is paste_frame / paste_value of mask_paste_common.h (contraction off inside them).
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void paste_rotated_masks_kernel(PasteParams p) {
  const int r = blockIdx.z;
  const int py = blockIdx.y;
  const PasteFrame f = paste_frame(p.boxes + (long)r * 5, p.M);
  const float* mk = p.masks + (long)r * p.M * p.M;
  uint8_t* orow = p.out + ((long)r * p.H + py) * p.W;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q * 4 < p.W; q += gridDim.x * blockDim.x) {
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int px = q * 4 + k;
      uint32_t bit = 0;
      if (px < p.W) {
        const float v = paste_value(f, mk, p.M, px, py);
        // threshold >= 0: boolean mask; threshold < 0: the reference's visualisation mode, (v * 255).to(uint8)
        const float v255 = v * 255.f;
        bit = p.threshold >= 0.f ? ((v >= p.threshold) ? 1u : 0u) : ((uint32_t)(int)v255 & 0xffu);
      }
      packed |= bit << (8 * k);
    }
    if (q * 4 + 3 < p.W && (((uintptr_t)(orow + q * 4)) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(orow + q * 4) = packed;
    } else {
      for (int k = 0; k < 4; ++k)
        if (q * 4 + k < p.W) orow[q * 4 + k] = (uint8_t)((packed >> (8 * k)) & 0xff);
    }
  }
}

}  // namespace

extern "C" int glass_pixel_shuffle2x_nhwc(const float* x, float* y, int N, int H, int W, int C, glass_stream_t stream) {
  GLASS_CHECK_ARG(x && y, "glass_pixel_shuffle2x_nhwc: null pointer");
  GLASS_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "glass_pixel_shuffle2x_nhwc: C=%d must be a positive multiple of 4", C);
  if (N == 0) return GLASS_OK;
  const long total = (long)N * H * W * C;      // float4 count of the input (= 4 * C/4 per pixel)
  hipLaunchKernelGGL(pixel_shuffle2x_kernel, dim3(grid_for_n(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), N, H, W, C / 4);
  GLASS_CHECK_LAUNCH("glass_pixel_shuffle2x_nhwc");
  return GLASS_OK;
}

extern "C" int glass_sigmoid_inplace(float* x, int64_t n, glass_stream_t stream) {
  GLASS_CHECK_ARG(x != nullptr || n == 0, "glass_sigmoid_inplace: null pointer");
  if (n <= 0) return GLASS_OK;
  hipLaunchKernelGGL(sigmoid_kernel, dim3(grid_for_n(n, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)n);
  GLASS_CHECK_LAUNCH("glass_sigmoid_inplace");
  return GLASS_OK;
}

extern "C" int glass_paste_rotated_masks(const float* masks, const float* boxes, int R, int M, int H, int W, float threshold,
                                         uint8_t* out, glass_stream_t stream) {
  GLASS_CHECK_ARG(R == 0 || (masks && boxes && out), "glass_paste_rotated_masks: null pointer");
  GLASS_CHECK_ARG(R >= 0 && M > 0 && H > 0 && W > 0 && H <= 65535 && R <= 65535, "glass_paste_rotated_masks: bad dims");
  if (R == 0) return GLASS_OK;
  PasteParams p{masks, boxes, out, R, M, H, W, threshold};
  const int quads = (W + 3) / 4;
  hipLaunchKernelGGL(paste_rotated_masks_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)H, (unsigned)R), dim3(256), 0,
                     (hipStream_t)stream, p);
  GLASS_CHECK_LAUNCH("glass_paste_rotated_masks");
  return GLASS_OK;
}
