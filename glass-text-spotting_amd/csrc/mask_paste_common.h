// The rotated mask paste as device functions: one pixel of the reference's paste_masks_in_image / _do_paste_mask
// (glass/postprocess/post_processor_academic.py:187-335), shared by the paste kernel (csrc/masks.hip), which writes the whole
// [R][H][W] tensor, and by the mask polygoniser (csrc/mask_rings.hip), which evaluates it where it needs a pixel.
#pragma once
#include <hip/hip_runtime.h>

// what the paste needs of one box [5] (cx, cy, w, h, angle in degrees)
struct PasteFrame {
  float cx, cy, cs, sn, nsn, x0, y0, dx, dy, halfM;
};

// BIT-EXACT against the reference's torch-CPU path (tests/golden/mask_paste.npz, produced by the reference's own
// paste_masks_in_image): every fp32 operation below is the one torch executes, in its order, with fusion exactly where
// torch's kernels fuse (established by emulation, oracle/README notes + tests/test_mask_branch.py):
//   * `stack([gx, gy]) @ rot` is an sgemm with K = 2: acc = gx * r0; acc = fma(gy, r1, acc);
//   * the following `+= c`, `- x0`, `/ (x1 - x0)`, `* 2`, `- 1` are separate elementwise kernels (each rounded);
//   * grid_sample (CPU, vectorised): unnormalise = fma(n + 1, M / 2, -0.5); weights e = 1 - w, s = 1 - n,
//     nw = e*s, ne = w*s, sw = e*n, se = w*n; out = nw_v*nw, then fma(ne_v, ne, out), fma(sw_v, sw, out), fma(se_v, se, out)
//     with out-of-range taps contributing a value of 0 (masked gather);
//   * cos / sin: correctly rounded fp32 (evaluated in fp64 and rounded), which is what torch's SLEEF kernels return
//     for all but rare inputs.
// Compiler contraction is off inside both functions, wherever they are inlined; the fused operations are explicit
// __builtin_fmaf calls.
__device__ __forceinline__ PasteFrame paste_frame(const float* __restrict__ b, int M) {
#pragma clang fp contract(off)
  PasteFrame f;
  const float bw = b[2], bh = b[3];
  f.cx = b[0];
  f.cy = b[1];
  // torch.deg2rad multiplies by pi/180 in fp32
  const float ang = b[4] * 0.017453292519943295f;
  f.cs = (float)cos((double)ang);
  f.sn = (float)sin((double)ang);
  f.nsn = -f.sn;
  // x0 = cx + (h * sin_t - w * cos_t) / 2 with sin_t = 0, cos_t = 1 (python ints in the reference)
  const float x0 = f.cx + (bh * 0.f - bw * 1.f) / 2.f, x1 = f.cx - (bh * 0.f - bw * 1.f) / 2.f;
  const float y0 = f.cy - (bh * 1.f + bw * 0.f) / 2.f, y1 = f.cy + (bh * 1.f + bw * 0.f) / 2.f;
  f.x0 = x0;
  f.y0 = y0;
  f.dx = x1 - x0;
  f.dy = y1 - y0;
  f.halfM = (float)M / 2.f;
  return f;
}

// the bilinear sample of mask mk [M][M] at image pixel (px, py): 0 wherever the pixel's centre falls outside the box
// inflated by 1 + 1/M (floor(fx) or floor(fy) outside [-1, M)), and for a NaN anywhere on the way.  Every index into mk
// is checked against M.
__device__ __forceinline__ float paste_value(const PasteFrame& f, const float* __restrict__ mk, int M, int px, int py) {
#pragma clang fp contract(off)
  const float gy = ((float)py + 0.5f) - f.cy;
  const float gx = ((float)px + 0.5f) - f.cx;
  // [gx, gy] @ [[cos, sin], [-sin, cos]] (K = 2 sgemm), recentred, normalised to the box
  float ix = __builtin_fmaf(gy, f.nsn, gx * f.cs);
  float iy = __builtin_fmaf(gy, f.cs, gx * f.sn);
  ix = ix + f.cx;
  iy = iy + f.cy;
  float nx = (ix - f.x0) / f.dx;
  nx = nx * 2.f;
  nx = nx - 1.f;
  float ny = (iy - f.y0) / f.dy;
  ny = ny * 2.f;
  ny = ny - 1.f;
  // grid_sample, align_corners=False, bilinear, zero padding
  const float fx = __builtin_fmaf(nx + 1.f, f.halfM, -0.5f);
  const float fy = __builtin_fmaf(ny + 1.f, f.halfM, -0.5f);
  const float flx = floorf(fx), fly = floorf(fy);
  float v = 0.f;
  if (flx >= -1.f && flx < (float)M && fly >= -1.f && fly < (float)M) {   // (also false for NaN: v stays 0)
    const int xw = (int)flx, yn = (int)fly;
    const float tw = fx - flx, te = 1.f - tw, tn = fy - fly, ts = 1.f - tn;
    const float wnw = te * ts, wne = tw * ts, wsw = te * tn, wse = tw * tn;
    const bool xin0 = xw >= 0, xin1 = xw + 1 < M;
    const bool yin0 = yn >= 0, yin1 = yn + 1 < M;
    const float vnw = (yin0 && xin0) ? mk[yn * M + xw] : 0.f;
    const float vne = (yin0 && xin1) ? mk[yn * M + xw + 1] : 0.f;
    const float vsw = (yin1 && xin0) ? mk[(yn + 1) * M + xw] : 0.f;
    const float vse = (yin1 && xin1) ? mk[(yn + 1) * M + xw + 1] : 0.f;
    v = vnw * wnw;
    v = __builtin_fmaf(vne, wne, v);
    v = __builtin_fmaf(vsw, wsw, v);
    v = __builtin_fmaf(vse, wse, v);
  }
  return v;
}

// The candidate rectangle of a box: every pixel the paste can set lies inside it.  A pasted pixel is non-zero only where its
// centre p + 0.5 lies in the box inflated by 1 + 1/M; with A = |w|/2 (1 + 1/M), B = |h|/2 (1 + 1/M) the rotated box spans
// ex = A|cos| + B|sin|, ey = A|sin| + B|cos| around (cx, cy).  Evaluated in double, widened by PASTE_RECT_MARGIN pixels on
// every side (the paste itself rounds in fp32), clipped to the image WHILE STILL IN DOUBLE, and only then turned into
// integers: nothing of a box reaches an index unclipped.  (x0, y0, x1, y1) inclusive; (W, H, -1, -1) = empty, also for a box
// with a non-finite component (the paste yields 0 everywhere for those: a NaN fails its range test).
// The margin is sized for boxes at image scale (|cx|, |cy|, |w|, |h| up to about 2^20, one float32 ulp well below a pixel);
// far beyond that the float32 paste can leave the float64 rectangle (include/glass_hip_feature_roimask.h states the limit).
constexpr int PASTE_RECT_MARGIN = 2;

__device__ __forceinline__ int4 paste_rect(const float* __restrict__ b, int M, int H, int W) {
  const int4 none = make_int4(W, H, -1, -1);
  const float c0 = b[0], c1 = b[1], c2 = b[2], c3 = b[3], c4 = b[4];
  if (!(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3) && isfinite(c4))) return none;
  const float ang = c4 * 0.017453292519943295f;
  if (!isfinite(ang)) return none;
  const double cs = fabs(cos((double)ang)), sn = fabs(sin((double)ang));
  const double grow = 1.0 + 1.0 / (double)M;
  const double A = fabs((double)c2) * 0.5 * grow, B = fabs((double)c3) * 0.5 * grow;
  const double ex = A * cs + B * sn, ey = A * sn + B * cs;
  const double m = (double)PASTE_RECT_MARGIN;
  double x0 = ceil((double)c0 - ex - 0.5) - m, x1 = floor((double)c0 + ex - 0.5) + m;
  double y0 = ceil((double)c1 - ey - 0.5) - m, y1 = floor((double)c1 + ey - 0.5) + m;
  x0 = fmax(x0, 0.0);
  y0 = fmax(y0, 0.0);
  x1 = fmin(x1, (double)(W - 1));
  y1 = fmin(y1, (double)(H - 1));
  if (!(x0 <= x1 && y0 <= y1)) return none;
  return make_int4((int)x0, (int)y0, (int)x1, (int)y1);
}
