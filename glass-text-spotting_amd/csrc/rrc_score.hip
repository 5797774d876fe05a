// RRC end-to-end protocol geometry (reference glass/evaluation/text_eval_script.py:98-120, 339-409): polygon areas, the
// intersection area of every (ground truth, detection) pair of every image, and the protocol's decisions on them
// (don't-care detections, greedy IoU matching) for the end-to-end and the detection-only care sets.
//
// Polygons are integer rings in CSR form (pts [P][2], poly_off [n_poly + 1]); an image is a range of GT polygon indices
// and a range of detection polygon indices; pair p of image i, row-major [G_i][D_i], lives at pair_off[i] + g * D_i + d.
//
// Intersection area: the indicator of a simple polygon is orient * sum_e sign_e * 1[T_e] (T_e the trapezoid between edge e
// and a horizontal baseline below the polygon, sign_e the direction of e along x), so
//   area(A n B) = orient_A * orient_B * sum_{e in A, f in B} sign_e * sign_f * area(T_e n T_f),
// and area(T_e n T_f) = integral of min(line_e, line_f) over the common x range of the two edges
//   = integral of (a + b) / 2  -  integral of |a - b| / 2,
// both closed forms of the four end heights (the crossing abscissa is never formed).  No clipping, no sorting, any
// orientation, convex or not; vertical and zero-length edges (a closed ring's repeated first point) contribute nothing.
// Origin and baseline are the lower corner of the pair's joint bounding box: shifted coordinates are exact small integers
// and every height is >= 0.  All arithmetic is fp64.
//
// Work split of glass_rrc_pair_areas: each lane of a wave first takes one pair and tests the bounding boxes (disjoint:
// exactly 0.0, no edge is read).  The surviving pairs of the wave are then served by groups of lanes that stride over the
// ne * nf edge pairs: RRC_GROUP lanes (4 pairs at a time) when ne * nf <= RRC_BIG_PAIR, the whole wave otherwise.  The
// group size depends on the pair alone, every lane sums its terms in index order with a compensated (Kahan) sum and the
// lanes combine in a fixed xor-shuffle tree, so a result does not depend on the grid, on the neighbours in the wave or on
// scheduling: two runs are bit-identical.  No atomics, no waiting on another workgroup, every loop bounded by a size read
// once.
#include <climits>
#include "common.h"

namespace {

constexpr int RRC_THREADS = 256;
constexpr int RRC_WAVES = RRC_THREADS / 64;
constexpr int RRC_GROUP = 16;            // lanes per small pair: a quad pair has 16 edge pairs
constexpr int RRC_BIG_PAIR = 1024;       // more edge pairs than this: the whole wave serves the pair

// one thread per polygon: area = |shoelace| / 2 (int64, exact), orientation sign, bounding box (empty: min > max)
__global__ void rrc_polygon_kernel(const int2* __restrict__ pts, long P, const int* __restrict__ poly_off, int n_poly,
                                   double* __restrict__ area, int4* __restrict__ bbox, int* __restrict__ orient) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_poly) return;
  const long b = min(max((long)poly_off[k], 0l), P);
  const long e = min(max((long)poly_off[k + 1], b), P);
  long long a2 = 0;
  int4 bb = make_int4(INT_MAX, INT_MAX, INT_MIN, INT_MIN);
  if (e > b) {
    int2 p = pts[e - 1];
    for (long i = b; i < e; ++i) {
      const int2 q = pts[i];
      a2 += (long long)p.x * q.y - (long long)q.x * p.y;
      bb.x = min(bb.x, q.x);
      bb.y = min(bb.y, q.y);
      bb.z = max(bb.z, q.x);
      bb.w = max(bb.w, q.y);
      p = q;
    }
  }
  area[k] = (double)(a2 < 0 ? -a2 : a2) * 0.5;
  bbox[k] = bb;
  orient[k] = a2 > 0 ? 1 : (a2 < 0 ? -1 : 0);
}

// sign_e * sign_f * integral over the common x range of min(line_e, line_f); e = (x1,y1)-(x2,y2), f = (u1,v1)-(u2,v2)
__device__ __forceinline__ double edge_pair_term(double x1, double y1, double x2, double y2, double u1, double v1, double u2,
                                                 double v2) {
  if (x1 == x2 || u1 == u2) return 0.0;
  const double lo = fmax(fmin(x1, x2), fmin(u1, u2));
  const double hi = fmin(fmax(x1, x2), fmax(u1, u2));
  if (!(hi > lo)) return 0.0;
  const double me = (y2 - y1) / (x2 - x1), mf = (v2 - v1) / (u2 - u1);
  const double a0 = y1 + (lo - x1) * me, a1 = y1 + (hi - x1) * me;
  const double b0 = v1 + (lo - u1) * mf, b1 = v1 + (hi - u1) * mf;
  const double dx = hi - lo;
  const double d0 = a0 - b0, d1 = a1 - b1;
  const double p0 = fabs(d0), p1 = fabs(d1);
  const bool cross = (d0 > 0.0 && d1 < 0.0) || (d0 < 0.0 && d1 > 0.0);
  const double absint = cross ? dx * ((d0 * d0 + d1 * d1) / (2.0 * (p0 + p1))) : dx * ((p0 + p1) * 0.5);
  const double t = ((a0 + a1) + (b0 + b1)) * 0.25 * dx - 0.5 * absint;
  return ((x2 > x1) == (u2 > u1)) ? t : -t;
}

// this lane's share (edge pairs sl, sl + GROUP, ...) of pair (g, d); all lanes of a group get the group's total
template <int GROUP>
__device__ __forceinline__ double pair_intersection(const int2* __restrict__ pts, long P, const int* __restrict__ poly_off,
                                                    const int4* __restrict__ bbox, const int* __restrict__ orient, int g, int d,
                                                    int sl, bool active) {
  double sum = 0.0, comp = 0.0;
  double sgn = 0.0;
  if (active) {
    const long ea = min(max((long)poly_off[g], 0l), P), fa = min(max((long)poly_off[d], 0l), P);
    const unsigned ne = (unsigned)(min(max((long)poly_off[g + 1], ea), P) - ea);
    const unsigned nf = (unsigned)(min(max((long)poly_off[d + 1], fa), P) - fa);
    const int4 bg = bbox[g], bd = bbox[d];
    const int ox = min(bg.x, bd.x), oy = min(bg.y, bd.y);
    sgn = (double)(orient[g] * orient[d]);
    const unsigned long long n = (unsigned long long)ne * nf;
    for (unsigned long long k = (unsigned)sl; k < n; k += GROUP) {
      const unsigned ie = (unsigned)(k / nf), jf = (unsigned)(k - (unsigned long long)ie * nf);
      const int2 e1 = pts[ea + ie], e2 = pts[ea + (ie + 1 == ne ? 0 : ie + 1)];
      const int2 f1 = pts[fa + jf], f2 = pts[fa + (jf + 1 == nf ? 0 : jf + 1)];
      const double t = edge_pair_term((double)(e1.x - ox), (double)(e1.y - oy), (double)(e2.x - ox), (double)(e2.y - oy),
                                      (double)(f1.x - ox), (double)(f1.y - oy), (double)(f2.x - ox), (double)(f2.y - oy));
      const double y = t - comp;                                       // Kahan: the sum's error does not grow with ne * nf
      const double s = sum + y;
      comp = (s - sum) - y;
      sum = s;
    }
  }
#pragma unroll
  for (int off = GROUP / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  return fmax(sgn * sum, 0.0);
}

__global__ __launch_bounds__(RRC_THREADS) void rrc_pair_inter_kernel(
    const int2* __restrict__ pts, long P, const int* __restrict__ poly_off, int n_poly, const int* __restrict__ gt_off,
    const int* __restrict__ det_off, const long long* __restrict__ pair_off, int I, long long n_pairs,
    const int4* __restrict__ bbox, const int* __restrict__ orient, double* __restrict__ inter) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long stride = (long long)gridDim.x * RRC_WAVES * 64;
  for (long long base = ((long long)blockIdx.x * RRC_WAVES + wid) * 64; base < n_pairs; base += stride) {   // wave-uniform
    const long long p = base + lane;
    int g = 0, d = 0;
    bool overlap = false, big = false;
    if (p < n_pairs) {
      int lo = 0, hi = I;                                              // the image: last i with pair_off[i] <= p
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid;
      }
      const int g0 = gt_off[lo], d0 = det_off[lo];
      const long long D = max(det_off[lo + 1] - d0, 1);
      const long long r = p - pair_off[lo];
      g = g0 + (int)(r / D);
      d = d0 + (int)(r % D);
      if (g >= 0 && g < n_poly && d >= 0 && d < n_poly) {
        const int4 bg = bbox[g], bd = bbox[d];
        overlap = min(bg.z, bd.z) > max(bg.x, bd.x) && min(bg.w, bd.w) > max(bg.y, bd.y);
        if (overlap)
          big = (long long)(poly_off[g + 1] - poly_off[g]) * (poly_off[d + 1] - poly_off[d]) > RRC_BIG_PAIR;
      }
      if (!overlap) inter[p] = 0.0;
    }
    unsigned long long big_mask = __ballot(big);
    unsigned long long small_mask = __ballot(overlap) & ~big_mask;
    while (small_mask) {                                               // 64 / RRC_GROUP pairs per turn
      unsigned long long m = small_mask;
      const int sub = lane / RRC_GROUP;
      for (int j = 0; j < sub; ++j) m &= m - 1;
      const bool active = m != 0;
      const int src = active ? __ffsll((long long)m) - 1 : 0;
      const int gg = __shfl(g, src), dd = __shfl(d, src);
      const double v = pair_intersection<RRC_GROUP>(pts, P, poly_off, bbox, orient, gg, dd, lane % RRC_GROUP, active);
      if (active && lane % RRC_GROUP == 0) inter[base + src] = v;
      for (int j = 0; j < 64 / RRC_GROUP && small_mask; ++j) small_mask &= small_mask - 1;
    }
    while (big_mask) {
      const int src = __ffsll((long long)big_mask) - 1;
      const int gg = __shfl(g, src), dd = __shfl(d, src);
      const double v = pair_intersection<64>(pts, P, poly_off, bbox, orient, gg, dd, lane, true);
      if (lane == 0) inter[base + src] = v;
      big_mask &= big_mask - 1;
    }
  }
}

// one workgroup per image.  Phase 1, all threads over detections: the don't-care marks of the two care sets.  Phase 2,
// wave 0 (end-to-end set) and wave 1 (detection-only set): the reference's greedy pass, serial over GT, lanes over
// detections, lowest detection index first (ballot + first set bit per 64-chunk).
__global__ __launch_bounds__(RRC_THREADS) void rrc_match_kernel(
    const double* __restrict__ area, int n_poly, const double* __restrict__ inter, long long n_pairs,
    const long long* __restrict__ pair_off, const int* __restrict__ gt_off, const int* __restrict__ det_off, int I,
    const unsigned char* __restrict__ gt_dc_e2e, const unsigned char* __restrict__ gt_dc_det, int n_gt, int n_det,
    unsigned char* det_dc_e2e, unsigned char* det_dc_det, int* __restrict__ match_e2e, int* __restrict__ match_det,
    unsigned char* taken) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int gbase = gt_off[0], dbase = det_off[0];
  for (int img = blockIdx.x; img < I; img += gridDim.x) {
    const int g0 = gt_off[img], d0 = det_off[img];
    const int G = gt_off[img + 1] - g0, D = det_off[img + 1] - d0;
    const long long base = pair_off[img];
    // uniform over the workgroup: an image whose ranges leave the arrays is skipped whole (the host never builds one)
    if (G < 0 || D < 0 || g0 < 0 || d0 < 0 || (long)g0 + G > n_poly || (long)d0 + D > n_poly || g0 - gbase < 0 ||
        g0 - gbase + G > n_gt || d0 - dbase < 0 || d0 - dbase + D > n_det || base < 0 || base + (long long)G * D > n_pairs)
      continue;
    for (int d = tid; d < D; d += RRC_THREADS) {
      const double ad = area[d0 + d];
      unsigned char e = 0, t = 0;
      for (int g = 0; g < G; ++g) {
        const unsigned char fe = gt_dc_e2e[g0 - gbase + g], ft = gt_dc_det[g0 - gbase + g];
        if (fe | ft) {
          const double ratio = ad == 0.0 ? 0.0 : inter[base + (long long)g * D + d] / ad;
          if (ratio > 0.5) {
            e |= fe ? 1 : 0;
            t |= ft ? 1 : 0;
          }
        }
      }
      det_dc_e2e[d0 - dbase + d] = e;
      det_dc_det[d0 - dbase + d] = t;
      taken[d0 - dbase + d] = 0;
      taken[(long)n_det + d0 - dbase + d] = 0;
    }
    __syncthreads();                                                   // phase 1's marks are visible to waves 0 and 1
    if (wid < 2) {
      const unsigned char* gt_dc = (wid ? gt_dc_det : gt_dc_e2e) + (g0 - gbase);
      const unsigned char* det_dc = (wid ? det_dc_det : det_dc_e2e) + (d0 - dbase);
      unsigned char* tk = taken + (wid ? (long)n_det : 0l) + (d0 - dbase);
      int* match = (wid ? match_det : match_e2e) + (g0 - gbase);
      for (int g = 0; g < G; ++g) {
        int m = -1;
        if (!gt_dc[g]) {                                          // uniform over the wave
          const double ag = area[g0 + g];
          for (int c = 0; c < D; c += 64) {
            const int d = c + lane;                                    // a detection is always seen by the same lane
            bool ok = false;
            if (d < D && !det_dc[d] && !tk[d]) {
              const double in = inter[base + (long long)g * D + d];
              const double un = ag + area[d0 + d] - in;
              ok = (un == 0.0 ? 0.0 : in / un) > 0.5;
            }
            const unsigned long long b = __ballot(ok);
            if (b) {
              const int first = __ffsll((long long)b) - 1;
              m = c + first;
              if (lane == first) tk[d] = 1;
              break;
            }
          }
        }
        if (lane == 0) match[g] = m;
      }
    }
    __syncthreads();
  }
}

constexpr long RRC_MAX_POINTS = 1l << 30;

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int64_t glass_rrc_pair_areas_workspace_bytes(int n_poly) {
  return n_poly > 0 ? align16((int64_t)n_poly * 16) + align16((int64_t)n_poly * 4) : 0;
}

extern "C" int glass_rrc_pair_areas(const int* pts, int64_t n_points, const int* poly_off, int n_poly, const int* gt_off,
                                    const int* det_off, const int64_t* pair_off, int n_images, int64_t n_pairs, double* area,
                                    double* inter, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(n_points >= 0 && n_points <= RRC_MAX_POINTS && n_poly >= 0 && n_images >= 0 && n_pairs >= 0,
                  "glass_rrc_pair_areas: bad sizes n_points=%lld n_poly=%d n_images=%d n_pairs=%lld", (long long)n_points, n_poly,
                  n_images, (long long)n_pairs);
  if (n_poly == 0) {
    GLASS_CHECK_ARG(n_pairs == 0, "glass_rrc_pair_areas: %lld pairs but no polygon", (long long)n_pairs);
    return GLASS_OK;
  }
  GLASS_CHECK_ARG(poly_off && area && workspace && (pts || n_points == 0), "glass_rrc_pair_areas: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)pts & 7) == 0, "glass_rrc_pair_areas: pts must be 8-byte aligned");
  GLASS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "glass_rrc_pair_areas: workspace must be 16-byte aligned");
  GLASS_CHECK_ARG(workspace_bytes >= glass_rrc_pair_areas_workspace_bytes(n_poly),
                  "glass_rrc_pair_areas: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
                  (long long)glass_rrc_pair_areas_workspace_bytes(n_poly));
  if (n_pairs > 0)
    GLASS_CHECK_ARG(n_images > 0 && gt_off && det_off && pair_off && inter, "glass_rrc_pair_areas: %lld pairs need images and offsets",
                    (long long)n_pairs);
  hipStream_t st = (hipStream_t)stream;
  int4* bbox = static_cast<int4*>(workspace);
  int* orient = reinterpret_cast<int*>(static_cast<char*>(workspace) + align16((int64_t)n_poly * 16));
  hipLaunchKernelGGL(rrc_polygon_kernel, dim3(cdiv(n_poly, 256)), dim3(256), 0, st, reinterpret_cast<const int2*>(pts), (long)n_points,
                     poly_off, n_poly, area, bbox, orient);
  GLASS_CHECK_LAUNCH("glass_rrc_pair_areas (polygons)");
  if (n_pairs > 0) {
    const long long blocks = (n_pairs + RRC_WAVES * 64 - 1) / (RRC_WAVES * 64);
    hipLaunchKernelGGL(rrc_pair_inter_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(RRC_THREADS), 0, st,
                       reinterpret_cast<const int2*>(pts), (long)n_points, poly_off, n_poly, gt_off, det_off,
                       reinterpret_cast<const long long*>(pair_off), n_images, (long long)n_pairs, bbox, orient, inter);
    GLASS_CHECK_LAUNCH("glass_rrc_pair_areas");
  }
  return GLASS_OK;
}

extern "C" int64_t glass_rrc_match_workspace_bytes(int n_det) { return n_det > 0 ? align16((int64_t)n_det * 2) : 0; }

extern "C" int glass_rrc_match(const double* area, int n_poly, const double* inter, int64_t n_pairs, const int64_t* pair_off,
                               const int* gt_off, const int* det_off, int n_images, const uint8_t* gt_dontcare_e2e,
                               const uint8_t* gt_dontcare_det, int n_gt, int n_det, uint8_t* det_dontcare_e2e,
                               uint8_t* det_dontcare_det, int* match_e2e, int* match_det, void* workspace, int64_t workspace_bytes,
                               glass_stream_t stream) {
  GLASS_CHECK_ARG(n_poly >= 0 && n_pairs >= 0 && n_images >= 0 && n_gt >= 0 && n_det >= 0 && (int64_t)n_gt + n_det <= n_poly,
                  "glass_rrc_match: bad sizes n_poly=%d n_pairs=%lld n_images=%d n_gt=%d n_det=%d", n_poly, (long long)n_pairs,
                  n_images, n_gt, n_det);
  if (n_images == 0 || (n_gt == 0 && n_det == 0)) return GLASS_OK;
  GLASS_CHECK_ARG(area && pair_off && gt_off && det_off, "glass_rrc_match: null pointer");
  GLASS_CHECK_ARG(n_gt == 0 || (gt_dontcare_e2e && gt_dontcare_det && match_e2e && match_det), "glass_rrc_match: null GT array");
  GLASS_CHECK_ARG(n_det == 0 || (det_dontcare_e2e && det_dontcare_det && workspace), "glass_rrc_match: null detection array");
  GLASS_CHECK_ARG(n_pairs == 0 || inter, "glass_rrc_match: null inter");
  GLASS_CHECK_ARG(workspace_bytes >= glass_rrc_match_workspace_bytes(n_det), "glass_rrc_match: workspace of %lld bytes, needs %lld",
                  (long long)workspace_bytes, (long long)glass_rrc_match_workspace_bytes(n_det));
  hipLaunchKernelGGL(rrc_match_kernel, dim3((unsigned)(n_images < 65536 ? n_images : 65536)), dim3(RRC_THREADS), 0,
                     (hipStream_t)stream, area, n_poly, inter, (long long)n_pairs, reinterpret_cast<const long long*>(pair_off), gt_off,
                     det_off, n_images, gt_dontcare_e2e, gt_dontcare_det, n_gt, n_det, det_dontcare_e2e, det_dontcare_det, match_e2e,
                     match_det, static_cast<unsigned char*>(workspace));
  GLASS_CHECK_LAUNCH("glass_rrc_match");
  return GLASS_OK;
}
