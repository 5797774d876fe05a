// Detected words grouped into text lines in reading order (include/glass_hip_feature_lines.h states the contract;
// glass_amd/postprocess/line_grouping.py:group_lines_host is the same statement in numpy float64).
//
// Two launches, the second ordered after the first by the stream:
//   lg_pairs_kernel   one wavefront per (image, 64-word row block), so the quadratic part spreads over the chip: the image's
//                     words are staged in LDS with their reading directions (float64 cos / sin, once per word), then lane =
//                     column word j, a loop over the block's rows i, and the ballot of Link(i, j) is the 64-bit row word
//                     rel[i][j / 64] in the workspace (ceil(K / 64) words per row; 128 KB per image at K = 1024).  A
//                     conservative float64 reject (centres farther apart than the sum of the two words' reach) skips the
//                     far-apart pairs before the four tests, as pp_far_apart does for the IoU.
//   lg_lines_kernel   one workgroup of 1024 threads per image, thread = word: components by hooking with integer minimum
//                     atomics in LDS (the fixed point labels every word with its component's smallest index, whatever the
//                     order of the atomics), the page frame by a fixed 1024-slot tree sum, each line's frame and box by its
//                     root thread walking the members in index order, ranks of lines and of words by counting smaller keys.
// All arithmetic is float64 without fused multiply-add, there are no float atomics, and nothing here waits for the host.
// Rows beyond the count are never read, and every index taken from memory (a bit of a row word, a label) is checked or is
// by construction one of 0 .. 1023, the size of the LDS arrays.
#include "common.h"
#include "glass_hip_feature_lines.h"

#pragma clang fp contract(off)

constexpr int LG_KMAX = GLASS_GROUP_LINES_MAX_K;
constexpr int LG_THREADS = 1024;
static_assert(LG_THREADS == LG_KMAX && LG_KMAX % 64 == 0, "one thread per word; the tree sum covers LG_KMAX slots");

struct LGParams { double max_angle, min_hr, max_off, max_gap; };

__host__ __device__ inline int lg_row_words(int K) { return (K + 63) / 64; }
__host__ __device__ inline long lg_image_words(int K) { return ((long)K * lg_row_words(K) + 1) / 2 * 2; }   // 64-bit words, a 16-byte multiple

struct LGWord { double cx, cy, w, h, a, ux, uy; bool valid; };

// one word from its row: widened exactly, valid iff all five finite and w, h > 0; u = (cos t, -sin t), t = a pi / 180
__device__ inline LGWord lg_load(const float* b) {
  const float f0 = b[0], f1 = b[1], f2 = b[2], f3 = b[3], f4 = b[4];
  LGWord q;
  q.valid = isfinite(f0) && isfinite(f1) && isfinite(f2) && isfinite(f3) && isfinite(f4) && f2 > 0.f && f3 > 0.f;
  q.cx = (double)f0; q.cy = (double)f1; q.w = (double)f2; q.h = (double)f3; q.a = (double)f4;
  q.ux = 1.0; q.uy = 0.0;
  if (q.valid) {
    const double t = q.a * 3.14159265358979323846 / 180.0;
    q.ux = cos(t); q.uy = -sin(t);
  }
  return q;
}

__device__ __forceinline__ int lg_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ------------------------------------------------------------------------------------------------ the pair stage
__global__ __launch_bounds__(64) void lg_pairs_kernel(const float* __restrict__ boxes, const int* __restrict__ count, int K, LGParams p,
                                                      unsigned long long* __restrict__ ws) {
  __shared__ double s_cx[LG_KMAX], s_cy[LG_KMAX], s_ux[LG_KMAX], s_uy[LG_KMAX];       // 32 KB
  __shared__ float s_w[LG_KMAX], s_h[LG_KMAX], s_a[LG_KMAX];                          // 12 KB; s_w = -1: not a valid word
  const int img = blockIdx.y, rb = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  if (rb * 64 >= n) return;
  const float* gb = boxes + (long)img * K * 5;
  for (int j = lane; j < n; j += 64) {
    const LGWord q = lg_load(gb + 5 * j);
    s_cx[j] = q.cx; s_cy[j] = q.cy; s_ux[j] = q.ux; s_uy[j] = q.uy;
    s_w[j] = q.valid ? (float)q.w : -1.f; s_h[j] = (float)q.h; s_a[j] = (float)q.a;
  }
  __syncthreads();
  const int W = lg_row_words(K), nb = (n + 63) / 64;
  unsigned long long* rel = ws + (long)img * lg_image_words(K);
  const int rows = min(64, n - rb * 64);
  const double reach = p.max_gap + p.max_off;                 // a word reaches w / 2 + reach * h from its centre
  for (int jb = 0; jb < nb; ++jb) {
    const int j = jb * 64 + lane;
    const bool jv = j < n && s_w[j] > 0.f;
    const int js = jv ? j : 0;
    const double cxj = s_cx[js], cyj = s_cy[js], uxj = s_ux[js], uyj = s_uy[js];
    const double wj = (double)s_w[js], hj = (double)s_h[js], aj = (double)s_a[js];
    const double rho_j = wj / 2 + reach * hj;
    unsigned long long mine = 0ull;
    for (int ii = 0; ii < rows; ++ii) {
      const int i = rb * 64 + ii;                             // (wavefront-uniform: the reads of word i are broadcasts)
      bool link = false;
      const double wi = (double)s_w[i];
      if (jv && wi > 0 && i != j) {
        const double hi = (double)s_h[i];
        const double dx = cxj - s_cx[i], dy = cyj - s_cy[i];
        const double rho = (wi / 2 + reach * hi) + rho_j;
        // Link needs |d.u_i| <= (w_i + w_j) / 2 + max_gap H and |d.v_i| <= max_offset H, so |d| <= their sum <= rho
        if (!(dx * dx + dy * dy > rho * rho * (1.0 + 1e-9))) {
          const double uxi = s_ux[i], uyi = s_uy[i];
          double r = fmod(fabs(aj - (double)s_a[i]), 360.0);
          if (r > 180.0) r = 360.0 - r;
          const double H = fmax(hi, hj), h = fmin(hi, hj);
          const double half = (wi + wj) / 2;
          link = r <= p.max_angle && h >= p.min_hr * H &&
                 fabs(dx * -uyi + dy * uxi) <= p.max_off * H && fabs(dx * -uyj + dy * uxj) <= p.max_off * H &&
                 fabs(dx * uxi + dy * uyi) - half <= p.max_gap * H && fabs(dx * uxj + dy * uyj) - half <= p.max_gap * H;
        }
      }
      const unsigned long long m = __ballot(link);
      if (lane == ii) mine = m;
    }
    if (lane < rows) rel[(long)(rb * 64 + lane) * W + jb] = mine;
  }
}

// ------------------------------------------------------------------------------------------------ the per-image stage
// is line (root) j ahead of line (root) t: valid lines first by (m.P_V, m.P_U, root), then the invalid words by index
__device__ __forceinline__ bool lg_line_before(int j, int t, bool vj, bool vt, double a1, double a2, double b1, double b2) {
  if (vj != vt) return vj;
  if (!vj) return j < t;
  if (a1 != b1) return a1 < b1;
  if (a2 != b2) return a2 < b2;
  return j < t;
}

__global__ __launch_bounds__(LG_THREADS) void lg_lines_kernel(const float* __restrict__ boxes, const int* __restrict__ count, int K,
                                                              const unsigned long long* __restrict__ ws, int* __restrict__ line_id,
                                                              int* __restrict__ line_pos, int* __restrict__ order,
                                                              int* __restrict__ line_start, float* __restrict__ line_boxes,
                                                              int* __restrict__ line_count) {
  // 101 KB of static LDS: more than the 64 KB a workgroup may use on other parts, within the 160 KiB of a gfx950 CU (one
  // workgroup per CU; csrc/postprocess_dense.hip relies on the same).  The host checks the launch.
  __shared__ double s_cx[LG_KMAX], s_cy[LG_KMAX], s_ux[LG_KMAX], s_uy[LG_KMAX], s_w[LG_KMAX], s_h[LG_KMAX];    // 48 KB: the words
  __shared__ double s_lux[LG_KMAX], s_luy[LG_KMAX];       // a line's frame U, at its root (before: the tree sum of w u)
  __shared__ double s_k1[LG_KMAX], s_k2[LG_KMAX];         // a line's keys m.P_V and m.P_U, at its root (before: the tree sum of w)
  __shared__ double s_proj[LG_KMAX];                      // c_i . U of the word's line
  __shared__ int s_label[LG_KMAX], s_lrank[LG_KMAX], s_wline[LG_KMAX];
  __shared__ unsigned char s_valid[LG_KMAX];
  __shared__ int s_changed;
  const int img = blockIdx.x, t = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  const float* gb = boxes + (long)img * K * 5;

  // ---- the words; the page frame's sums over a fixed tree of LG_KMAX slots (zeros for what is no valid word)
  {
    LGWord q{0., 0., 0., 0., 0., 1., 0., false};
    if (t < n) q = lg_load(gb + 5 * t);
    s_cx[t] = q.cx; s_cy[t] = q.cy; s_ux[t] = q.ux; s_uy[t] = q.uy; s_w[t] = q.w; s_h[t] = q.h;
    s_valid[t] = q.valid ? 1 : 0;
    s_label[t] = t;
    s_lux[t] = q.valid ? q.w * q.ux : 0.0;
    s_luy[t] = q.valid ? q.w * q.uy : 0.0;
    s_k1[t] = q.valid ? q.w : 0.0;
  }
  __syncthreads();
  for (int stride = LG_KMAX / 2; stride > 0; stride >>= 1) {
    if (t < stride) { s_lux[t] += s_lux[t + stride]; s_luy[t] += s_luy[t + stride]; s_k1[t] += s_k1[t + stride]; }
    __syncthreads();
  }
  double PUx = 1.0, PUy = 0.0;
  {
    const double Dx = s_lux[0], Dy = s_luy[0], Sw = s_k1[0];
    const double nrm = sqrt(Dx * Dx + Dy * Dy);
    if (nrm > 1e-12 * Sw) { PUx = Dx / nrm; PUy = Dy / nrm; }
  }
  const bool valid = t < n && s_valid[t];

  // ---- components: hook the larger label under the smaller along every set bit, then shortcut, until a round changes
  // nothing.  Labels only decrease and stay indices of the component, so the loop ends, and it ends with every word of a
  // component labelled with the component's smallest index.
  const int W = lg_row_words(K), nb = (n + 63) / 64;
  // the word's row of the relation, read once (all words in flight together) and kept in registers for every round, with
  // the bits that are no neighbour - the word itself, anything from the count on, a word that is not valid - taken out
  constexpr int LG_ROW_WORDS = LG_KMAX / 64;
  unsigned long long rw[LG_ROW_WORDS];
  {
    const unsigned long long* row = ws + (long)img * lg_image_words(K) + (long)t * W;
#pragma unroll
    for (int jb = 0; jb < LG_ROW_WORDS; ++jb) rw[jb] = (valid && jb < nb) ? row[jb] : 0ull;
#pragma unroll
    for (int jb = 0; jb < LG_ROW_WORDS; ++jb) {
      unsigned long long m = rw[jb], keep = 0ull;
      while (m) {
        const int b = __ffsll((long long)m) - 1, j = jb * 64 + b;
        m &= m - 1;
        if (j < n && j != t && s_valid[j]) keep |= 1ull << b;
      }
      rw[jb] = keep;
    }
  }
  for (;;) {
    __syncthreads();
    if (t == 0) s_changed = 0;
    __syncthreads();
    {
      bool ch = false;
#pragma unroll
      for (int jb = 0; jb < LG_ROW_WORDS; ++jb) {
        unsigned long long m = rw[jb];
        while (m) {
          const int j = jb * 64 + __ffsll((long long)m) - 1;          // (< n: checked above)
          m &= m - 1;
          const int lj = lg_ld(&s_label[j]), lt = lg_ld(&s_label[t]);
          if (lj < lt) { atomicMin(&s_label[lt], lj); atomicMin(&s_label[t], lj); ch = true; }
          else if (lt < lj) { atomicMin(&s_label[lj], lt); atomicMin(&s_label[j], lt); ch = true; }
        }
      }
      if (ch) s_changed = 1;
    }
    __syncthreads();
    if (valid) {
      const int l = lg_ld(&s_label[t]), ll = lg_ld(&s_label[l]);
      if (ll < l) { atomicMin(&s_label[t], ll); s_changed = 1; }
    }
    __syncthreads();
    if (!s_changed) break;
  }
  const int lab = t < n ? s_label[t] : t;
  const bool is_root = t < n && lab == t;
  const int first = t & ~63;                                // (the wavefront's first word: members of its roots start there)

  // ---- the line's frame and box, by its root over the members in index order
  double mx = 0, my = 0, eu = 0, ev = 0, ang = 0;
  if (is_root && valid) {
    // (in the loops over j below j is wavefront-uniform, so every LDS read is a broadcast; the reads do not depend on a
    // branch, so that an unrolled loop has them all in flight and waits for the LDS once per eight words, not once per word)
    double Dx = 0, Dy = 0, Sw = 0;
#pragma unroll 8
    for (int j = first; j < n; ++j) {
      const bool mine = s_label[j] == t;
      const double wj = s_w[j], pxj = wj * s_ux[j], pyj = wj * s_uy[j];
      if (mine) { Dx += pxj; Dy += pyj; Sw += wj; }
    }
    const double nrm = sqrt(Dx * Dx + Dy * Dy);
    double Ux = s_ux[t], Uy = s_uy[t];
    if (nrm > 1e-12 * Sw) { Ux = Dx / nrm; Uy = Dy / nrm; }
    s_lux[t] = Ux; s_luy[t] = Uy;
    const double Vx = -Uy, Vy = Ux;
    double umin = 0, umax = 0, vmin = 0, vmax = 0;
    bool any = false;
#pragma unroll 4
    for (int j = first; j < n; ++j) {
      const bool mine = s_label[j] == t;
      const double uxj = s_ux[j], uyj = s_uy[j], hw = s_w[j] / 2, hh = s_h[j] / 2, cxj = s_cx[j], cyj = s_cy[j];
      if (mine) {
        const double ax = hw * uxj, ay = hw * uyj, bx = hh * -uyj, by = hh * uxj;       // (w / 2) u and (h / 2) v
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double su = (c & 1) ? -1.0 : 1.0, sv = (c & 2) ? -1.0 : 1.0;
          const double px = cxj + su * ax + sv * bx, py = cyj + su * ay + sv * by;
          const double pu = px * Ux + py * Uy, pv = px * Vx + py * Vy;
          if (!any) { umin = umax = pu; vmin = vmax = pv; any = true; }
          else { umin = fmin(umin, pu); umax = fmax(umax, pu); vmin = fmin(vmin, pv); vmax = fmax(vmax, pv); }
        }
      }
    }
    const double cu = (umin + umax) / 2, cv = (vmin + vmax) / 2;
    mx = cu * Ux + cv * Vx; my = cu * Uy + cv * Vy;
    eu = umax - umin; ev = vmax - vmin;
    ang = atan2(-Uy, Ux) * 180.0 / 3.14159265358979323846;
    s_k1[t] = mx * -PUy + my * PUx;                          // m . P_V
    s_k2[t] = mx * PUx + my * PUy;                           // m . P_U
  }
  __syncthreads();
  s_proj[t] = valid ? s_cx[t] * s_lux[lab] + s_cy[t] * s_luy[lab] : 0.0;

  // ---- rank of the line among the lines, by counting
  const int n_lines = __syncthreads_count(is_root);
  if (is_root) {
    int r = 0;
    const double b1 = s_k1[t], b2 = s_k2[t];
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const bool root_j = s_label[j] == j, vj = s_valid[j] != 0;
      const double a1 = s_k1[j], a2 = s_k2[j];                 // (whatever the tree sum left there where j is no valid root)
      r += (root_j && j != t && lg_line_before(j, t, vj, valid, a1, a2, b1, b2)) ? 1 : 0;
    }
    s_lrank[t] = r;
  }
  __syncthreads();
  s_wline[t] = t < n ? s_lrank[lab] : 0;
  __syncthreads();

  // ---- rank of the word among the words by (line, c.U, index); the outputs
  const long o = (long)img * K;
  if (t < n) {
    const int lt = s_wline[t];
    const double pt = s_proj[t];
    int rank = 0, ahead = 0;                                  // `ahead`: words of earlier lines = the line's start
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const int lj = s_wline[j];
      const double pj = s_proj[j];
      ahead += lj < lt ? 1 : 0;
      rank += (lj == lt && (pj < pt || (pj == pt && j < t))) ? 1 : 0;
    }
    order[o + ahead + rank] = t;
    line_id[o + t] = lt;
    line_pos[o + t] = rank;
    if (is_root) {
      line_start[(long)img * (K + 1) + lt] = ahead;
      float* lb = line_boxes + (o + lt) * 5;
      if (valid) { lb[0] = (float)mx; lb[1] = (float)my; lb[2] = (float)eu; lb[3] = (float)ev; lb[4] = (float)ang; }
      else {
        const unsigned* src = reinterpret_cast<const unsigned*>(gb + 5 * t);
        unsigned* dst = reinterpret_cast<unsigned*>(lb);
        for (int e = 0; e < 5; ++e) dst[e] = src[e];
      }
    }
  } else if (t < K) {
    order[o + t] = -1; line_id[o + t] = -1; line_pos[o + t] = -1;
  }
  if (t >= n_lines && t < K)
    for (int e = 0; e < 5; ++e) line_boxes[(o + t) * 5 + e] = 0.f;
  for (int e = n_lines + t; e <= K; e += LG_THREADS) line_start[(long)img * (K + 1) + e] = n;
  if (t == 0) line_count[img] = n_lines;
}

extern "C" int64_t glass_group_lines_workspace_bytes(int N, int K) {
  if (N < 0 || K < 0 || K > LG_KMAX) return -1;
  return (int64_t)N * lg_image_words(K) * 8;
}

extern "C" int glass_group_lines(const float* boxes, const int* count, int N, int K, const double* params4_host, int* line_id,
                                 int* line_pos, int* order, int* line_start, float* line_boxes, int* line_count, void* workspace,
                                 int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(N >= 0, "glass_group_lines: N=%d", N);
  GLASS_CHECK_ARG(K >= 0 && K <= LG_KMAX, "glass_group_lines: K=%d (max %d)", K, LG_KMAX);
  GLASS_CHECK_ARG(params4_host, "glass_group_lines: null parameters");
  LGParams p{params4_host[0], params4_host[1], params4_host[2], params4_host[3]};
  GLASS_CHECK_ARG(p.max_angle >= 0 && p.max_angle <= 180, "glass_group_lines: max_angle_diff=%g (0..180)", p.max_angle);
  GLASS_CHECK_ARG(p.min_hr >= 0 && p.min_hr <= 1, "glass_group_lines: min_height_ratio=%g (0..1)", p.min_hr);
  GLASS_CHECK_ARG(p.max_off >= 0 && p.max_off <= 1.7e308, "glass_group_lines: max_offset=%g (finite, >= 0)", p.max_off);
  GLASS_CHECK_ARG(p.max_gap >= 0 && p.max_gap <= 1.7e308, "glass_group_lines: max_gap=%g (finite, >= 0)", p.max_gap);
  if (N == 0) return GLASS_OK;
  GLASS_CHECK_ARG(count && line_start && line_count, "glass_group_lines: null pointer");
  GLASS_CHECK_ARG(K == 0 || (boxes && line_id && line_pos && order && line_boxes), "glass_group_lines: null pointer");
  const int64_t need = glass_group_lines_workspace_bytes(N, K);
  GLASS_CHECK_ARG(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need),
                  "glass_group_lines: workspace of %lld bytes (16-byte aligned), needs %lld", (long long)workspace_bytes,
                  (long long)need);
  if (K > 0) {
    hipLaunchKernelGGL(lg_pairs_kernel, dim3(lg_row_words(K), N), dim3(64), 0, (hipStream_t)stream, boxes, count, K, p,
                       static_cast<unsigned long long*>(workspace));
    GLASS_CHECK_LAUNCH("glass_group_lines (pairs)");
  }
  hipLaunchKernelGGL(lg_lines_kernel, dim3(N), dim3(LG_THREADS), 0, (hipStream_t)stream, boxes, count, K,
                     static_cast<const unsigned long long*>(workspace), line_id, line_pos, order, line_start, line_boxes, line_count);
  GLASS_CHECK_LAUNCH("glass_group_lines (lines)");
  return GLASS_OK;
}
