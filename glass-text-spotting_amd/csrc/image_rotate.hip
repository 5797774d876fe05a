// PIL.Image.rotate(angle, BILINEAR, expand=True, fillcolor) of a uint8 HWC image byte for byte, and rotated boxes through the
// same matrix (include/glass_hip_feature_rotate.h states the contract; glass_amd/data/transforms.py::rotate_u8_host and
// RotationTransform.map_rotated_boxes are the statements in numpy float64):
//   glass_rotate_u8:    one launch; a workgroup makes a 32 x 32 tile of the output, a wavefront 32 x 8 pixels of it, a thread four
//                       neighbouring pixels of a row, stored as three dwords where the twelve bytes lie inside the row.  The source
//                       is gathered straight from global memory: a wavefront's footprint is a rotated 32 x 8 rectangle, a few
//                       cache lines at any angle.
//   glass_rotate_boxes: a thread per box.
// Every formula is evaluated in float64 without contraction, in the order of the statement.  Every source index is clipped into
// the image before it is used.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "glass_hip_feature_rotate.h"

#pragma clang fp contract(off)

constexpr int RT_TX = 8;      // threads along x of a workgroup: 8 groups of 4 pixels = 32 pixels
constexpr int RT_TY = 32;     // rows of a workgroup: a wavefront is 8 threads x 8 rows
constexpr int RT_PX = 4;      // pixels of a thread: 12 bytes = 3 dwords

struct RtMatrix { double m[6]; };

// the three bytes of the output pixel (x, y) of the affine bilinear form
__device__ __forceinline__ void rt_affine_pixel(const uint8_t* __restrict__ src, int H, int W, const RtMatrix& M, int x, int y,
                                                const uint8_t fill[3], uint8_t px[3]) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  double xin = M.m[0] * xc + M.m[1] * yc + M.m[2];
  double yin = M.m[3] * xc + M.m[4] * yc + M.m[5];
  if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
    px[0] = fill[0]; px[1] = fill[1]; px[2] = fill[2];
    return;
  }
  xin -= 0.5;
  yin -= 0.5;
  const double fx = floor(xin), fy = floor(yin);       // in [-1, W - 1] and [-1, H - 1]
  const double dx = xin - fx, dy = yin - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), ya = min(max(y0, 0), H - 1);
  const bool below = y0 + 1 >= 0 && y0 + 1 < H;
  const uint8_t* r0 = src + (long)ya * W * 3;
  const uint8_t* r1 = src + (long)(below ? y0 + 1 : ya) * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a = (double)r0[xa * 3 + c], b = (double)r0[xb * 3 + c];
    const double v1 = a + (b - a) * dx;
    double v2 = v1;
    if (below) {
      const double p = (double)r1[xa * 3 + c], q = (double)r1[xb * 3 + c];
      v2 = p + (q - p) * dx;
    }
    const double v = v1 + (v2 - v1) * dy;
    px[c] = (uint8_t)(int)v;
  }
}

// the three bytes of the output pixel (x, y) of a copy or transpose; 0 <= x < Wo, 0 <= y < Ho, so the source index is inside
__device__ __forceinline__ void rt_transpose_pixel(const uint8_t* __restrict__ src, int H, int W, int kind, int x, int y,
                                                   uint8_t px[3]) {
  int sx, sy;
  if (kind == 0) { sx = x; sy = y; }
  else if (kind == 1) { sx = W - 1 - y; sy = x; }
  else if (kind == 2) { sx = W - 1 - x; sy = H - 1 - y; }
  else { sx = y; sy = H - 1 - x; }
  sx = min(max(sx, 0), W - 1);
  sy = min(max(sy, 0), H - 1);
  const uint8_t* p = src + ((long)sy * W + sx) * 3;
  px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
}

// Row y of dst starts at byte dst + y * Wo * 3, on any alignment.  Its pixels are cut into groups of four that start on a dword:
// a group's first byte is (row start) + 3 * xs, a multiple of 4 iff xs == (row start) mod 4, so group g of the row covers the
// pixels [s - 4 + 4 g, s + 4 g) with s = (row start) & 3; the first and the last group of a row may be partial.
template <bool AFFINE>
__global__ __launch_bounds__(RT_TX * RT_TY) void rt_rotate_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                                  uint8_t* __restrict__ dst, int Ho, int Wo, RtMatrix M, int kind,
                                                                  int fill_rgb) {
  const int g = blockIdx.x * RT_TX + threadIdx.x;
  const uint8_t fill[3] = {(uint8_t)(fill_rgb & 255), (uint8_t)((fill_rgb >> 8) & 255), (uint8_t)((fill_rgb >> 16) & 255)};
  for (long y = (long)blockIdx.y * RT_TY + threadIdx.y; y < Ho; y += (long)gridDim.y * RT_TY) {
    uint8_t* row = dst + y * Wo * 3;
    const int s = (int)((uintptr_t)row & 3);
    const long xs = (long)s - RT_PX + (long)RT_PX * g;        // the group's first pixel: may be negative, or past the row
    if (xs >= Wo) continue;
    uint8_t b[RT_PX * 3];
#pragma unroll
    for (int i = 0; i < RT_PX; ++i) {
      const long x = xs + i;
      if (x >= 0 && x < Wo) {
        if (AFFINE) rt_affine_pixel(src, H, W, M, (int)x, (int)y, fill, b + 3 * i);
        else rt_transpose_pixel(src, H, W, kind, (int)x, (int)y, b + 3 * i);
      } else {
        b[3 * i] = b[3 * i + 1] = b[3 * i + 2] = 0;
      }
    }
    if (xs >= 0 && xs + RT_PX <= Wo) {                         // whole: three aligned dwords
      uint32_t* q = reinterpret_cast<uint32_t*>(row + xs * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        q[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) | ((uint32_t)b[4 * k + 3] << 24);
    } else {                                                   // an end of the row: its own bytes only
#pragma unroll
      for (int i = 0; i < RT_PX; ++i) {
        const long x = xs + i;
        if (x >= 0 && x < Wo) {
          uint8_t* q = row + x * 3;
          q[0] = b[3 * i]; q[1] = b[3 * i + 1]; q[2] = b[3 * i + 2];
        }
      }
    }
  }
}

static bool rt_finite6(const double* m) {
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(m[i])) return false;
  return true;
}

extern "C" int glass_rotate_u8(const uint8_t* src, int H, int W, uint8_t* dst, int Ho, int Wo, const double* matrix6_host, int kind,
                               int fill_r, int fill_g, int fill_b, glass_stream_t stream) {
  const char* what = "glass_rotate_u8";
  GLASS_CHECK_ARG(H >= 0 && W >= 0 && Ho >= 0 && Wo >= 0, "%s: bad sizes %dx%d -> %dx%d", what, H, W, Ho, Wo);
  GLASS_CHECK_ARG((int64_t)H * W * 3 < ((int64_t)1 << 31) && (int64_t)Ho * Wo * 3 < ((int64_t)1 << 31),
                  "%s: image too large (%dx%d -> %dx%d): needs H*W*3 and Ho*Wo*3 below 2^31", what, H, W, Ho, Wo);
  GLASS_CHECK_ARG(kind >= 0 && kind <= 4, "%s: kind %d outside 0..4", what, kind);
  if (kind == 0 || kind == 2) GLASS_CHECK_ARG(Ho == H && Wo == W, "%s: kind %d keeps the size, got %dx%d -> %dx%d", what, kind, H, W, Ho, Wo);
  if (kind == 1 || kind == 3) GLASS_CHECK_ARG(Ho == W && Wo == H, "%s: kind %d swaps the sides, got %dx%d -> %dx%d", what, kind, H, W, Ho, Wo);
  GLASS_CHECK_ARG(matrix6_host, "%s: null matrix", what);
  GLASS_CHECK_ARG(rt_finite6(matrix6_host), "%s: a matrix entry is not finite", what);
  GLASS_CHECK_ARG(fill_r >= 0 && fill_r <= 255 && fill_g >= 0 && fill_g <= 255 && fill_b >= 0 && fill_b <= 255,
                  "%s: fill (%d, %d, %d) outside 0..255", what, fill_r, fill_g, fill_b);
  if ((int64_t)H * W == 0 || (int64_t)Ho * Wo == 0) return GLASS_OK;
  GLASS_CHECK_ARG(src && dst, "%s: null image", what);
  RtMatrix M;
  for (int i = 0; i < 6; ++i) M.m[i] = matrix6_host[i];
  const int groups = cdiv((long)Wo + RT_PX, RT_PX);            // the shifted grouping needs at most one more than Wo / 4
  const int rows = cdiv(Ho, RT_TY);
  const dim3 grid((unsigned)cdiv(groups, RT_TX), (unsigned)(rows < 65535 ? rows : 65535)), block(RT_TX, RT_TY);
  const int fill = fill_r | (fill_g << 8) | (fill_b << 16);
  if (kind == 4)
    hipLaunchKernelGGL(rt_rotate_kernel<true>, grid, block, 0, (hipStream_t)stream, src, H, W, dst, Ho, Wo, M, kind, fill);
  else
    hipLaunchKernelGGL(rt_rotate_kernel<false>, grid, block, 0, (hipStream_t)stream, src, H, W, dst, Ho, Wo, M, kind, fill);
  GLASS_CHECK_LAUNCH(what);
  return GLASS_OK;
}

// ---------------------------------------------------------------- boxes
__global__ __launch_bounds__(256) void rt_boxes_kernel(const float* boxes, int n, RtMatrix M, double theta, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float f[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) f[k] = boxes[(long)i * 5 + k];
  const double big = (double)INFINITY;
  const bool finite = fabs((double)f[0]) < big && fabs((double)f[1]) < big && fabs((double)f[2]) < big && fabs((double)f[3]) < big &&
                      fabs((double)f[4]) < big;                  // a NaN fails its comparison
  if (finite) {
    const double cx = f[0], cy = f[1];
    double a = (double)f[4] + theta;
    a = a - 360.0 * floor((a + 180.0) / 360.0);
    f[0] = (float)(M.m[0] * cx + M.m[1] * cy + M.m[2]);
    f[1] = (float)(M.m[3] * cx + M.m[4] * cy + M.m[5]);
    f[4] = (float)a;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) out[(long)i * 5 + k] = f[k];
}

extern "C" int glass_rotate_boxes(const float* boxes, int n, const double* matrix6_host, double theta_degrees, float* out,
                                  glass_stream_t stream) {
  const char* what = "glass_rotate_boxes";
  GLASS_CHECK_ARG(n >= 0 && n <= (1 << 26), "%s: n = %d", what, n);
  GLASS_CHECK_ARG(matrix6_host, "%s: null matrix", what);
  GLASS_CHECK_ARG(rt_finite6(matrix6_host) && std::isfinite(theta_degrees), "%s: a matrix entry or theta is not finite", what);
  if (n == 0) return GLASS_OK;
  GLASS_CHECK_ARG(boxes && out, "%s: null pointer", what);
  RtMatrix M;
  for (int i = 0; i < 6; ++i) M.m[i] = matrix6_host[i];
  hipLaunchKernelGGL(rt_boxes_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, boxes, n, M, theta_degrees, out);
  GLASS_CHECK_LAUNCH(what);
  return GLASS_OK;
}
