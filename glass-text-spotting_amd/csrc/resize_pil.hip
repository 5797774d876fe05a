// PIL.Image.resize(BILINEAR) of a uint8 HWC image, byte for byte (include/glass_hip.h "PIL bilinear resize"): two separable
// integer passes with host-made 22-bit fixed-point coefficient tables, a uint8 intermediate [H,Wo,3] between them, and -
// for the model's front end - a vertical pass that stores the normalised pixel straight into a slot of the NHWC4 batch.
// Threads run along x in both passes: the vertical pass reads whole rows of its source coalesced (its coefficient row is
// the same for the whole block, so it comes through the scalar cache) and its float4 / 3-byte stores are contiguous.
// Integer work only, up to the final convert.  The kernels clamp every table row to its axis, so a table that does not
// belong to the sizes of the call gives wrong pixels, never an access outside the image.
#include "common.h"

#define RP_PREC 22                   // PIL's PRECISION_BITS = 32 - 8 - 2
#define RP_BLOCK 256

__device__ __forceinline__ int rp_clip8(int acc) {
  const int v = acc >> RP_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// first tap and tap count of table row `o`, clamped to [0, in) and to the table's row length
__device__ __forceinline__ void rp_bounds(const int* __restrict__ bounds, int o, int in, int ksize, int& first, int& n) {
  first = bounds[2 * o];
  n = bounds[2 * o + 1];
  first = first < 0 ? 0 : (first > in ? in : first);
  n = n > ksize ? ksize : n;
  n = n > in - first ? in - first : n;
}

// ---------------------------------------------------------------- horizontal pass: [H,W,3] -> [H,Wo,3]
// one thread per output pixel (3 channels), blockIdx.y strides over the rows
__global__ __launch_bounds__(RP_BLOCK) void resize_pil_x_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                                const int* __restrict__ kx, const int* __restrict__ bx,
                                                                int ksize, uint8_t* __restrict__ dst, int Wo) {
  const int xo = blockIdx.x * RP_BLOCK + threadIdx.x;
  if (xo >= Wo) return;
  int x0, n;
  rp_bounds(bx, xo, W, ksize, x0, n);
  const int* k = kx + (long)xo * ksize;
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    const uint8_t* p = src + ((long)y * W + x0) * 3;
    int a0 = 1 << (RP_PREC - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int c = k[t];
      a0 += c * p[3 * t]; a1 += c * p[3 * t + 1]; a2 += c * p[3 * t + 2];
    }
    uint8_t* q = dst + ((long)y * Wo + xo) * 3;
    q[0] = (uint8_t)rp_clip8(a0); q[1] = (uint8_t)rp_clip8(a1); q[2] = (uint8_t)rp_clip8(a2);
  }
}

// ---------------------------------------------------------------- vertical pass: [Hi,Wo,3] -> [Ho,Wo,3] or the batch slot
// ky == nullptr: the axis keeps its size, the pass is a copy (and, into the batch, the normalisation alone).
// TO_BATCH: the grid covers the padded slot [Hp,Wp]; out = float4 slot base, pixels outside [Ho,Wo] and channel 3 are 0.
template <bool TO_BATCH>
__global__ __launch_bounds__(RP_BLOCK) void resize_pil_y_kernel(const uint8_t* __restrict__ src, int Hi, int Wo,
                                                                const int* __restrict__ ky, const int* __restrict__ by,
                                                                int ksize, void* __restrict__ out, int Ho, int rows, int cols,
                                                                float m0, float m1, float m2, float s0, float s1, float s2,
                                                                int flip) {
  const int x = blockIdx.x * RP_BLOCK + threadIdx.x;
  if (x >= cols) return;
  for (int yo = blockIdx.y; yo < rows; yo += gridDim.y) {
    int a0 = 0, a1 = 0, a2 = 0;
    const bool inside = yo < Ho && x < Wo;
    if (inside) {
      if (ky) {
        int y0, n;
        rp_bounds(by, yo, Hi, ksize, y0, n);
        const int* k = ky + (long)yo * ksize;
        const uint8_t* p = src + ((long)y0 * Wo + x) * 3;
        a0 = a1 = a2 = 1 << (RP_PREC - 1);
        for (int t = 0; t < n; ++t, p += (long)Wo * 3) {
          const int c = k[t];
          a0 += c * p[0]; a1 += c * p[1]; a2 += c * p[2];
        }
        a0 = rp_clip8(a0); a1 = rp_clip8(a1); a2 = rp_clip8(a2);
      } else {
        const uint8_t* p = src + ((long)yo * Wo + x) * 3;
        a0 = p[0]; a1 = p[1]; a2 = p[2];
      }
    }
    if (TO_BATCH) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (inside) {             // the operation order of preprocess_kernel (elementwise.hip): subtract, then a true division
        v.x = ((float)(flip ? a2 : a0) - m0) / s0;
        v.y = ((float)a1 - m1) / s1;
        v.z = ((float)(flip ? a0 : a2) - m2) / s2;
      }
      static_cast<float4*>(out)[(long)yo * cols + x] = v;
    } else if (inside) {
      uint8_t* q = static_cast<uint8_t*>(out) + ((long)yo * Wo + x) * 3;
      q[0] = (uint8_t)a0; q[1] = (uint8_t)a1; q[2] = (uint8_t)a2;
    }
  }
}

static inline dim3 rp_grid(int cols, int rows) {
  return dim3((unsigned)cdiv(cols, RP_BLOCK), (unsigned)(rows < 65535 ? rows : 65535));
}

extern "C" int64_t glass_resize_pil_workspace_bytes(int H, int W, int Ho, int Wo) {
  (void)Ho;
  if (H <= 0 || W <= 0 || Wo <= 0 || W == Wo) return 0;
  return (int64_t)H * Wo * 3;
}

// the checks the two entry points share; the largest image is bounded so that every pixel index times 3 fits an int64
// with room and the row / column counts fit the 32-bit kernel arguments
static int rp_check(const char* what, const uint8_t* src, int H, int W, const int* kx, const int* bx, int ksize_x, const int* ky,
                    const int* by, int ksize_y, const void* workspace, int64_t workspace_bytes, int Ho, int Wo, bool need_ws) {
  GLASS_CHECK_ARG(src, "%s: null image", what);
  GLASS_CHECK_ARG(H > 0 && W > 0 && Ho > 0 && Wo > 0, "%s: bad sizes %dx%d -> %dx%d", what, H, W, Ho, Wo);
  GLASS_CHECK_ARG(H <= (1 << 24) && W <= (1 << 24) && Ho <= (1 << 24) && Wo <= (1 << 24), "%s: image too large", what);
  GLASS_CHECK_ARG(W == Wo || (kx && bx && ksize_x > 0), "%s: the width changes (%d -> %d) but there is no horizontal table", what, W, Wo);
  GLASS_CHECK_ARG(H == Ho || (ky && by && ksize_y > 0), "%s: the height changes (%d -> %d) but there is no vertical table", what, H, Ho);
  if (need_ws) {
    const int64_t need = glass_resize_pil_workspace_bytes(H, W, Ho, Wo);
    GLASS_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", what,
                    (long long)workspace_bytes, (long long)need);
  }
  return GLASS_OK;
}

extern "C" int glass_resize_u8_pil(const uint8_t* src, int H, int W, const int* kx, const int* bx, int ksize_x, const int* ky,
                                   const int* by, int ksize_y, void* workspace, int64_t workspace_bytes, uint8_t* dst, int Ho,
                                   int Wo, glass_stream_t stream) {
  const char* what = "glass_resize_u8_pil";
  const bool do_x = W != Wo, do_y = H != Ho;
  int rc = rp_check(what, src, H, W, kx, bx, ksize_x, ky, by, ksize_y, workspace, workspace_bytes, Ho, Wo, do_x && do_y);
  if (rc != GLASS_OK) return rc;
  GLASS_CHECK_ARG(dst, "%s: null output", what);
  hipStream_t s = (hipStream_t)stream;
  if (!do_x && !do_y) {
    if (hipMemcpyAsync(dst, src, (size_t)H * W * 3, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      glass_set_error("%s: copy failed", what);
      return GLASS_EHIP;
    }
    return GLASS_OK;
  }
  const uint8_t* mid = src;
  if (do_x) {                 // straight into the output when it is the only pass
    uint8_t* xo = do_y ? static_cast<uint8_t*>(workspace) : dst;
    hipLaunchKernelGGL(resize_pil_x_kernel, rp_grid(Wo, H), dim3(RP_BLOCK), 0, s, src, H, W, kx, bx, ksize_x, xo, Wo);
    GLASS_CHECK_LAUNCH(what);
    mid = xo;
  }
  if (do_y) {
    hipLaunchKernelGGL(resize_pil_y_kernel<false>, rp_grid(Wo, Ho), dim3(RP_BLOCK), 0, s, mid, H, Wo, ky, by, ksize_y,
                       (void*)dst, Ho, Ho, Wo, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 0);
    GLASS_CHECK_LAUNCH(what);
  }
  return GLASS_OK;
}

extern "C" int glass_resize_u8_pil_into_batch(const uint8_t* src, int H, int W, const int* kx, const int* bx, int ksize_x,
                                              const int* ky, const int* by, int ksize_y, void* workspace,
                                              int64_t workspace_bytes, int Ho, int Wo, const float* mean3, const float* std3,
                                              int flip_channels, float* batch_nhwc4, int n, int Hp, int Wp,
                                              glass_stream_t stream) {
  const char* what = "glass_resize_u8_pil_into_batch";
  const bool do_x = W != Wo, do_y = H != Ho;
  int rc = rp_check(what, src, H, W, kx, bx, ksize_x, ky, by, ksize_y, workspace, workspace_bytes, Ho, Wo, do_x);
  if (rc != GLASS_OK) return rc;
  GLASS_CHECK_ARG(mean3 && std3 && batch_nhwc4, "%s: null pointer", what);
  GLASS_CHECK_ARG(n >= 0 && Ho <= Hp && Wo <= Wp && Hp <= (1 << 24) && Wp <= (1 << 24), "%s: %dx%d does not fit slot %d of a %dx%d batch",
                  what, Ho, Wo, n, Hp, Wp);
  GLASS_CHECK_ARG(((uintptr_t)batch_nhwc4 & 15) == 0, "%s: the batch must be 16-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* mid = src;
  if (do_x) {
    hipLaunchKernelGGL(resize_pil_x_kernel, rp_grid(Wo, H), dim3(RP_BLOCK), 0, s, src, H, W, kx, bx, ksize_x,
                       static_cast<uint8_t*>(workspace), Wo);
    GLASS_CHECK_LAUNCH(what);
    mid = static_cast<const uint8_t*>(workspace);
  }
  float4* slot = reinterpret_cast<float4*>(batch_nhwc4) + (long)n * Hp * Wp;
  hipLaunchKernelGGL(resize_pil_y_kernel<true>, rp_grid(Wp, Hp), dim3(RP_BLOCK), 0, s, mid, H, Wo, do_y ? ky : nullptr,
                     do_y ? by : nullptr, ksize_y, (void*)slot, Ho, Hp, Wp, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                     std3[2], flip_channels);
  GLASS_CHECK_LAUNCH(what);
  return GLASS_OK;
}
