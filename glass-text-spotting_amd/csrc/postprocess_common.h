// The arithmetic of the word post-processor, shared by its two kernels: postprocess.hip (<= 128 boxes per image, everything
// in LDS) and postprocess_dense.hip (<= 1024 boxes, pair state in a global workspace).  Every function here is the one
// definition of a step of reference glass/postprocess/post_processor_rotated_boxes.py (see the header of postprocess.hip),
// so the two kernels produce the same bits wherever both apply.
#pragma once
#include "rotated_iou.h"

// No fused multiply-add anywhere in the post-processor: the reference computes these boxes with separate torch float32 ops and the
// pinned restatement of cv2.minAreaRect (glass_amd/postprocess/post_processor_rotated_boxes.py:min_area_rect) in numpy
// float64, neither of which fuses.  With hipcc's default (fuse wherever it can) WHICH product of `a*b + c*d` is fused
// depends on the surrounding code, so two builds of the same formulas differ by an ulp in one merge in a few thousand -
// enough to tip the choice between two equal-area hull edges, or a threshold test three merges later.
#pragma clang fp contract(off)

constexpr int PP_TMAX = 64;

struct PPParams {
  const float* boxes; const float* scores; const int* counts; const int* text_arg; const float* text_max; const float* scale_xy;
  int N, K, T;
  float min_box_dim, valid_score, detect_thr, merge_ioa, height_ratio, max_angle_diff, minimal_ioa, text_thr;
  int stop_index, do_text;
  float* out_boxes; float* out_scores; float* out_poly; int* out_src; int* out_char; float* out_text_score;
  int* out_text_len; int* out_count;
};

// ---- minimum-area enclosing rectangle of <= 8 points (double precision, same algorithm and tie order as
// glass_amd/postprocess/post_processor_rotated_boxes.py:min_area_rect): monotone-chain hull of the unique
// points sorted by (x, y), then the first hull edge of minimal bounding-rectangle area.
struct DPt { double x, y; };
__device__ inline double dcross(DPt o, DPt a, DPt b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// per-thread point lists in LDS: element i of column t at base[i * STRIDE + t] (conflict-free across a wavefront); STRIDE is
// the number of columns the kernel keeps (its thread count for the IoU's lists, its boxes in flight for the merge's)
template <int STRIDE>
struct LdsPtsT {
  Pt* base;
  __device__ __forceinline__ Pt& operator[](int i) const { return base[i * STRIDE]; }
};
template <int STRIDE>
struct LdsDPtsT {
  DPt* base;
  __device__ __forceinline__ DPt& operator[](int i) const { return base[i * STRIDE]; }
};

// Hull of the 8 corner points of two boxes.  `A`: 32 points of storage (sorted points 0..7, hull 8..23, upper chain 24..31);
// returns the number of hull points (<= 8).
template <int STRIDE>
__device__ int merge_hull(const float* pts /*[8][2]*/, LdsDPtsT<STRIDE> A) {
  const LdsDPtsT<STRIDE> p{A.base}, hull{A.base + 8 * STRIDE}, upper{A.base + 24 * STRIDE};
  int n = 8;
  for (int i = 0; i < 8; ++i) { p[i].x = (double)pts[2 * i]; p[i].y = (double)pts[2 * i + 1]; }
  // insertion sort by (x, y), then drop exact duplicates
  for (int i = 1; i < n; ++i) {
    const DPt key = p[i];
    int j = i - 1;
    while (j >= 0 && (p[j].x > key.x || (p[j].x == key.x && p[j].y > key.y))) { p[j + 1] = p[j]; --j; }
    p[j + 1] = key;
  }
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (m == 0 || p[i].x != p[m - 1].x || p[i].y != p[m - 1].y) p[m++] = p[i];
  n = m;
  int hn = 0;
  if (n <= 2) {
    for (int i = 0; i < n; ++i) hull[hn++] = p[i];
  } else {
    int nl = 0, nu = 0;                           // (the lower chain is built in place at the head of `hull`)
    for (int i = 0; i < n; ++i) {
      const DPt pi = p[i];
      while (nl >= 2 && dcross(hull[nl - 2], hull[nl - 1], pi) <= 0) --nl;
      hull[nl++] = pi;
    }
    for (int i = n - 1; i >= 0; --i) {
      const DPt pi = p[i];
      while (nu >= 2 && dcross(upper[nu - 2], upper[nu - 1], pi) <= 0) --nu;
      upper[nu++] = pi;
    }
    hn = nl - 1;
    for (int i = 0; i < nu - 1; ++i) hull[hn++] = upper[i];
  }
  return hn;
}

// bounding rectangle of the hull with one side along hull edge i (false: zero-length edge)
struct EdgeRect { double area, cx, cy, w, h, ang; };
template <int STRIDE>
__device__ bool hull_edge_rect(LdsDPtsT<STRIDE> hull, int hn, int i, EdgeRect& r) {
  const DPt a = hull[i], b = hull[(i + 1) % hn];
  const double ex = b.x - a.x, ey = b.y - a.y;
  const double nrm = hypot(ex, ey);
  if (nrm == 0) return false;
  const double ux = ex / nrm, uy = ey / nrm, vx = -uy, vy = ux;
  double pumin = 1e300, pumax = -1e300, pvmin = 1e300, pvmax = -1e300;
  for (int k = 0; k < hn; ++k) {
    const DPt hk = hull[k];
    const double pu = hk.x * ux + hk.y * uy, pv = hk.x * vx + hk.y * vy;
    pumin = fmin(pumin, pu); pumax = fmax(pumax, pu); pvmin = fmin(pvmin, pv); pvmax = fmax(pvmax, pv);
  }
  const double ww = pumax - pumin, hh = pvmax - pvmin;
  r.area = ww * hh;
  const double cu = (pumax + pumin) / 2, cv = (pvmax + pvmin) / 2;
  r.cx = ux * cu + vx * cv; r.cy = uy * cu + vy * cv; r.w = ww; r.h = hh;
  r.ang = atan2(uy, ux) * 57.29577951308232;
  return true;
}

__device__ inline float floor_mod_pp(float a, float b) {   // torch.remainder semantics
  float m = fmodf(a, b);
  if (m != 0.f && ((b < 0.f) != (m < 0.f))) m += b;
  return m;
}

__device__ inline double pymod(double a, double b) {   // Python float % for b > 0
  double m = fmod(a, b);
  if (m != 0 && m < 0) m += b;
  return m;
}

// boxes_to_polygons (:219-250) for one box, float32 like the reference's torch ops
__device__ inline void box_polygon(const float* b, float* poly /*[4][2]*/) {
  const float cx = b[0], cy = b[1], w = b[2], h = b[3], a = b[4];
  const float t = (-a / 180.f) * 3.14159265358979323846f;
  float s, c;
  sincosf(t, &s, &c);
  poly[0] = cx + (h * s - w * c) / 2;  poly[1] = cy - (h * c + w * s) / 2;
  poly[2] = cx + (h * s + w * c) / 2;  poly[3] = cy - (h * c - w * s) / 2;
  poly[4] = cx - (h * s - w * c) / 2;  poly[5] = cy + (h * c + w * s) / 2;
  poly[6] = cx - (h * s + w * c) / 2;  poly[7] = cy + (h * c - w * s) / 2;
}

// _merge_rotated_boxes (:187-216) + polygons_to_rotated_boxes (:253-286) for one pair, in two parts around the minimum-area
// rectangle (cx, cy, w, h, ang) of the pair's 8 corners: merge_corners before, merge_finish after
__device__ inline void merge_corners(const float* b1, const float* b2, float* pts /*[8][2]*/) {
  box_polygon(b1, pts);
  box_polygon(b2, pts + 8);
}
__device__ inline void merge_finish(const float* b1, const float* b2, float s1, float s2, double cx, double cy, double w, double h, double ang,
                                    float* out) {
  const float a1 = b1[4] * 3.14159265358979323846f / 180.f, a2 = b2[4] * 3.14159265358979323846f / 180.f;
  const double orient = (double)(s1 >= s2 ? a1 : a2);          // radians (reference quirk)
  double angle = 90.0 - ang;
  double diff = pymod((orient - angle) + 180.0, 360.0) - 180.0;
  double width, height;
  if (-45 < diff && diff <= 45) { width = h; height = w; }
  else if (45 < diff && diff <= 135) { width = w; height = h; angle += 90; }
  else if (-135 < diff && diff <= -45) { width = w; height = h; angle -= 90; }
  else { width = h; height = w; angle += 180; }
  angle = pymod(angle + 180.0, 360.0) - 180.0;
  out[0] = (float)cx; out[1] = (float)cy; out[2] = (float)width; out[3] = (float)height; out[4] = (float)angle;
}

// The load step of both kernels: RotatedBoxes.scale of the runner's un-scaling (skipped for a (1, 1) ratio like the
// reference's `if scale_ratio != 1`), in place on b[5]
__device__ inline void pp_unscale(float* b, float sx, float sy) {
  b[0] *= sx; b[1] *= sy;
  const float theta = b[4] * 3.14159265358979323846f / 180.0f;
  float sn, cs;
  sincosf(theta, &sn, &cs);
  b[2] *= sqrtf((sx * cs) * (sx * cs) + (sy * sn) * (sy * sn));
  b[3] *= sqrtf((sx * sn) * (sx * sn) + (sy * cs) * (sy * cs));
  b[4] = atan2f(sx * sn, sy * cs) * 180.0f / 3.14159265358979323846f;
}

// Circumscribed circles disjoint (with slack) -> the rectangles cannot intersect -> IoU is exactly 0; skips the
// polygon clipping for the (vast majority of) far-apart word pairs.
__device__ __forceinline__ bool pp_far_apart(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  const float r = 0.5f * (sqrtf(a[2] * a[2] + a[3] * a[3]) + sqrtf(b[2] * b[2] + b[3] * b[3]));
  return dx * dx + dy * dy > r * r * 1.001f + 1e-2f;
}

// The pair test of merge_intersecting_boxes (:118-160) for boxes i < j of the snapshot, given the pair's IoA
__device__ __forceinline__ bool pp_pair_valid(const PPParams& p, const float* bi, const float* bj, float si, float sj, float v) {
  if (!(v >= p.minimal_ioa)) return false;
  float ad = bj[4] - bi[4];
  ad = fabsf(floor_mod_pp(ad + 180.f, 360.f) - 180.f);
  const bool sim_angle = (ad < p.max_angle_diff) || (ad > (180.f - p.max_angle_diff));
  const float hr = bj[3] / bi[3];
  const bool sim_h = (p.height_ratio < hr) && (hr < (1.f / (p.height_ratio + 1e-6f)));
  const bool vs = fminf(si, sj) >= p.valid_score;
  return sim_angle && sim_h && vs && (v >= p.merge_ioa);
}

// pairwise_ioa_rotated (glass/structures/boxes.py:33-48) from the pair's IoU
__device__ __forceinline__ float pp_ioa_of(const float* bi, const float* bj, float iou) {
  const float a1 = bi[2] * bi[3], a2 = bj[2] * bj[3];
  const float inter = (a1 + a2) * iou / (1.f + iou);
  return inter / fminf(a1, a2);
}
