// Word post-processing on device for 128 < K <= 1024 padded detections per image ("dense" form of postprocess.hip).
//
// Same semantics, same arithmetic (postprocess_common.h, rotated_iou.h) and same order of the floating-point operations as
// postprocess_words_kernel, whose header states them: optional un-scaling, filter_small_boxes, score >= valid, the merge loop
// on a snapshot with "last valid pair as second element, else last valid pair as first element" write-back, the merged
// angle in radians into the degree-valued correction, the 0.99 NMS in stable descending score order with reordering of the
// survivors, word score / length from text_argmax_kernel's output, the detect / text thresholds, ordered compaction.
//
// What differs is where the pair state lives.  The 128-box kernel holds an n x n IoA / IoU matrix in LDS (66 KB); at 1024
// boxes that would be 4 MB.  But the matrix is only ever reduced: the merge needs, per box, the largest first index and the
// largest second index over its VALID pairs, and the NMS needs the pairs with IoU >= 0.99.  So one workgroup per image
// (512 threads, no synchronisation between workgroups) walks the pairs by rows, runs the polygon clipping only for the near
// ones (!pp_far_apart, collected 64 at a time per wavefront so the long path runs with all lanes busy) and keeps
//   * maxi[b], maxj[b]: integer atomicMax over the valid pairs (j == b resp. i == b);
//   * the list of (sorted position a < sorted position c) pairs with IoU >= 0.99, appended in whatever order the
//     wavefronts find them; the greedy suppression is then evaluated as the fixed point it defines ("c is removed iff some
//     kept a < c has a listed pair (a, c)"), which does not depend on the order of the list;
// both in the global workspace (L2-resident; sized for the worst case, K (K - 1) / 2 listed pairs).  Integer max and a fixed
// point are independent of the order in which the wavefronts get there, so results are identical from run to run.
// The workspace is read and written with agent-scope atomic accesses only: it is shared between the wavefronts of one
// workgroup across barriers, and must not be served from a stale line of the CU's vector cache.
//
// LDS: the boxes and their snapshot (2 x 20 KB), scores / half cos / half sin (12 KB), three 16-bit index arrays (6 KB), the
// wavefronts' near-pair queues (4 KB) and 96 KB for the 512 threads' IoU point lists (24 points x 8 B each; 1024 threads
// would need 192 KB, which the 160 KiB CU does not have).  The merge's hull lists (32 double points per box, 64 boxes per
// pass) and the suppression's state bytes reuse those 96 KB between barriers.
#include "postprocess_common.h"

#pragma clang fp contract(off)

constexpr int PD_KMAX = 1024;
constexpr int PD_THREADS = 512;
constexpr int PD_WAVES = PD_THREADS / 64;
constexpr int PD_SLOTS = PD_KMAX / PD_THREADS;            // positions per thread: tid + r * PD_THREADS
constexpr int PD_MERGE_BOXES = PD_THREADS / 8;            // eight lanes per merged box
constexpr int PD_WORK_BYTES = 24 * 8 * PD_THREADS;        // >= 32 DPt x PD_MERGE_BOXES, >= 3 x PD_KMAX state bytes
static_assert(PD_WORK_BYTES >= 32 * 16 * PD_MERGE_BOXES && PD_WORK_BYTES >= 3 * PD_KMAX, "work area");
static_assert(PD_SLOTS == 2 && PD_KMAX <= (1 << 10), "pair entries hold 10-bit indices; two positions per thread");

using PdPts = LdsPtsT<PD_THREADS>;
using PdDPts = LdsDPtsT<PD_MERGE_BOXES>;

__host__ __device__ inline long pd_hi_capacity(int K) { return (long)K * (K - 1) / 2; }
__host__ __device__ inline long pd_image_words(int K) { return ((2L * K + pd_hi_capacity(K)) + 3) / 4 * 4; }    // 16-byte multiple

__device__ __forceinline__ int pd_ws_load(const int* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pd_ws_store(int* q, int v) { __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Ordered compaction over the PD_KMAX positions (position tid + r * PD_THREADS on thread tid): dst[r] = number of kept
// positions below; returns the total.  Two barriers; whatever a thread read before the call may be overwritten after it.
__device__ __forceinline__ int pd_compact(const bool (&keep)[PD_SLOTS], int (&dst)[PD_SLOTS], int* s_wcnt /*[PD_SLOTS * PD_WAVES]*/, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  unsigned long long m[PD_SLOTS];
#pragma unroll
  for (int r = 0; r < PD_SLOTS; ++r) {
    m[r] = __ballot(keep[r]);
    if (lane == 0) s_wcnt[r * PD_WAVES + wave] = __popcll(m[r]);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int r = 0; r < PD_SLOTS; ++r) dst[r] = __popcll(m[r] & below);
#pragma unroll
  for (int k = 0; k < PD_SLOTS * PD_WAVES; ++k) {
    const int c = s_wcnt[k];
#pragma unroll
    for (int r = 0; r < PD_SLOTS; ++r)
      if (k < r * PD_WAVES + wave) dst[r] += c;
    total += c;
  }
  __syncthreads();
  return total;
}

// All pairs (i < j) of n boxes by rows (row i on wavefront i % PD_WAVES, 64 columns per trip): on_far(i, j) for the
// far-apart ones when `want_far`; the others are collected per wavefront (ballot compaction into `queue`, 128 entries) and
// handed to on_near(i, j) 64 at a time.  No triangular-index inversion: rows and columns are loop counters.
template <class Far, class Near>
__device__ __forceinline__ void pd_for_pairs(int n, const float (*B)[5], unsigned* queue, int tid, bool want_far, Far on_far, Near on_near) {
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int qn = 0;                                                       // (wavefront-uniform)
  for (int i = wave; i < n - 1; i += PD_WAVES) {
    for (int j0 = i + 1; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool near = false;
      if (j < n) {
        near = !pp_far_apart(B[i], B[j]);
        if (!near && want_far) on_far(i, j);
      }
      const unsigned long long m = __ballot(near);
      if (near) queue[qn + __popcll(m & below)] = ((unsigned)i << 10) | (unsigned)j;
      qn += __popcll(m);
      if (qn >= 64) {
        qn -= 64;
        const unsigned e = queue[qn + lane];
        on_near((int)(e >> 10), (int)(e & 1023u));
      }
    }
  }
  if (lane < qn) {
    const unsigned e = queue[lane];
    on_near((int)(e >> 10), (int)(e & 1023u));
  }
}

__global__ __launch_bounds__(PD_THREADS) void postprocess_words_dense_kernel(PPParams p, int* workspace) {
  __shared__ float bx[PD_KMAX][5], snap[PD_KMAX][5];
  __shared__ float sc[PD_KMAX], rc2[PD_KMAX], rs2[PD_KMAX];       // rc2 / rs2: make_rbox's half cos / sin of bx
  __shared__ unsigned short src[PD_KMAX], order[PD_KMAX], pos[PD_KMAX];
  __shared__ unsigned queue[PD_WAVES][128];
  __shared__ int s_wcnt[PD_SLOTS * PD_WAVES], s_hn[PD_MERGE_BOXES], s_n, s_any, s_hi_n, s_und;
  // the threads' IoU point lists / the merge's hull lists / the suppression's state bytes; the phases that use the three
  // views are separated by barriers
  __shared__ __attribute__((aligned(16))) unsigned char work[PD_WORK_BYTES];
  const int n_img = blockIdx.x, tid = threadIdx.x;
  const int K = p.K;
  const int cnt = min(p.counts[n_img], min(K, PD_KMAX));
  const float* gb = p.boxes + (long)n_img * K * 5;
  const float* gs = p.scores + (long)n_img * K;
  int* ws = workspace + (long)n_img * pd_image_words(K);
  int* maxi = ws;                    // [K] largest i of a valid pair (i, b), -1: none
  int* maxj = ws + K;                // [K] largest j of a valid pair (b, j), -1: none
  int* hi = ws + 2 * K;              // [K (K - 1) / 2] (a << 16 | c): sorted positions a < c with IoU >= 0.99
  const int hi_cap = (int)pd_hi_capacity(K);
  PdPts iou_pts{reinterpret_cast<Pt*>(work) + tid};
  unsigned char* state = work;                    // [PD_KMAX] 0 undecided, 1 kept, 2 removed
  unsigned char* mark_kept = work + PD_KMAX;      // [PD_KMAX] a kept earlier position suppresses this one
  unsigned char* mark_und = work + 2 * PD_KMAX;   // [PD_KMAX] an undecided earlier position could

  // ---- load (+ optional RotatedBoxes.scale of the runner's un-scaling), filter_small_boxes, score >= valid; survivors
  // compacted in order
  {
    float b[PD_SLOTS][5], sj[PD_SLOTS];
    bool keep[PD_SLOTS];
    int dst[PD_SLOTS];
#pragma unroll
    for (int r = 0; r < PD_SLOTS; ++r) {
      const int j = tid + r * PD_THREADS;
      keep[r] = false;
      sj[r] = 0.f;
#pragma unroll
      for (int e = 0; e < 5; ++e) b[r][e] = 0.f;
      if (j < cnt) {
        const float sx = p.scale_xy ? p.scale_xy[2 * n_img] : 1.f, sy = p.scale_xy ? p.scale_xy[2 * n_img + 1] : 1.f;
#pragma unroll
        for (int e = 0; e < 5; ++e) b[r][e] = gb[5 * j + e];
        sj[r] = gs[j];
        if (p.scale_xy && (sx != 1.f || sy != 1.f)) pp_unscale(b[r], sx, sy);     // GlassRunner un-scales only when the ratio != 1
        keep[r] = fminf(b[r][2], b[r][3]) >= p.min_box_dim && sj[r] >= p.valid_score;
      }
    }
    const int n0 = pd_compact(keep, dst, s_wcnt, tid);
#pragma unroll
    for (int r = 0; r < PD_SLOTS; ++r)
      if (keep[r]) {
        const int d = dst[r];
#pragma unroll
        for (int e = 0; e < 5; ++e) bx[d][e] = b[r][e];
        sc[d] = sj[r];
        src[d] = (unsigned short)(tid + r * PD_THREADS);
        const RBox rb = make_rbox(b[r][0], b[r][1], b[r][2], b[r][3], b[r][4]);
        rc2[d] = rb.c2; rs2[d] = rb.s2;
      }
    if (tid == 0) s_n = n0;
  }
  __syncthreads();
  auto rbox_of = [&](const float (*B)[5], int i) { return RBox{B[i][0], B[i][1], B[i][2], B[i][3], rc2[i], rs2[i]}; };
  // a far-apart pair has IoA exactly 0; it can only be a valid pair under thresholds <= 0
  const bool far_can_merge = 0.f >= p.minimal_ioa && 0.f >= p.merge_ioa;

  // ---- merge_intersecting_boxes
  const int iter_cap = 4 * K;
  for (int iter = 0; iter < iter_cap; ++iter) {
    const int n = s_n;
    if (n == 0) break;
    for (int i = tid; i < n * 5; i += PD_THREADS) snap[i / 5][i % 5] = bx[i / 5][i % 5];
    for (int i = tid; i < n; i += PD_THREADS) { pd_ws_store(maxi + i, -1); pd_ws_store(maxj + i, -1); }
    if (tid == 0) s_any = 0;
    __syncthreads();
    // valid pairs: IoA from the pair's IoU (same algebra as pairwise_ioa_rotated, glass/structures/boxes.py:33-48), then the
    // angle / height / score / IoA tests; rc2 / rs2 are those of bx = snap until the write-back
    auto valid_pair = [&](int i, int j, float v) {
      if (pp_pair_valid(p, snap[i], snap[j], sc[i], sc[j], v)) {
        atomicMax(maxi + j, i);
        atomicMax(maxj + i, j);
        s_any = 1;
      }
    };
    pd_for_pairs(n, snap, queue[tid >> 6], tid, far_can_merge, [&](int i, int j) { valid_pair(i, j, 0.f); },
                 [&](int i, int j) {
                   valid_pair(i, j, pp_ioa_of(snap[i], snap[j], rotated_iou_in(rbox_of(snap, i), rbox_of(snap, j), iou_pts)));
                 });
    __syncthreads();
    if (!s_any) break;
    // write-back: box b takes the merge of its LAST valid pair as second element (largest i), else of its last valid pair
    // as first element (largest j); all merges computed from the snapshot.  The boxes that take a merge are listed first
    // (in `order`, their partners in `pos`: both free until the NMS), then merged 64 per pass, eight lanes per box: lane 0
    // builds the hull of the pair's corners (LDS column), every lane evaluates the bounding rectangle along one hull edge
    // (<= 8), and the reference loop's choice - the first edge of strictly smaller area - is folded over the lanes' areas.
    int n_act;
    {
      bool act[PD_SLOTS];
      int partner[PD_SLOTS], dst[PD_SLOTS];
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r) {
        const int b = tid + r * PD_THREADS;
        partner[r] = -1;
        if (b < n) {
          partner[r] = pd_ws_load(maxi + b);
          if (partner[r] < 0) partner[r] = pd_ws_load(maxj + b);
        }
        act[r] = partner[r] >= 0;
      }
      n_act = pd_compact(act, dst, s_wcnt, tid);
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r)
        if (act[r]) { order[dst[r]] = (unsigned short)(tid + r * PD_THREADS); pos[dst[r]] = (unsigned short)partner[r]; }
    }
    __syncthreads();
    for (int a0 = 0; a0 < n_act; a0 += PD_MERGE_BOXES) {
      const int slot = tid >> 3, gl = tid & 7;
      const bool act = a0 + slot < n_act;
      const int b = act ? order[a0 + slot] : 0, q = act ? pos[a0 + slot] : 0;
      const int pi = min(b, q), pj = max(b, q);                  // (a pair is (smaller, larger) whichever element b is)
      const PdDPts A{reinterpret_cast<DPt*>(work) + slot}, hull{A.base + 8 * PD_MERGE_BOXES};
      if (act && gl == 0) {
        float pts[16];
        merge_corners(snap[pi], snap[pj], pts);
        s_hn[slot] = merge_hull(pts, A);
      }
      __syncthreads();
      const int hn = act ? s_hn[slot] : 0;
      EdgeRect r{0., 0., 0., 0., 0., 0.};
      const bool ok = act && hn >= 3 && gl < hn && hull_edge_rect(hull, hn, gl, r);
      int win = 0;
      double best = -1.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double ae = __shfl(r.area, e, 8);
        const int oke = __shfl((int)ok, e, 8);
        if (oke && (best < 0 || ae < best)) { best = ae; win = e; }
      }
      double cx = __shfl(r.cx, win, 8), cy = __shfl(r.cy, win, 8), w = __shfl(r.w, win, 8), h = __shfl(r.h, win, 8),
             ang = __shfl(r.ang, win, 8);
      if (act && gl == 0) {
        if (hn == 1) {
          const DPt h0 = hull[0];
          cx = h0.x; cy = h0.y; w = 0; h = 0; ang = 0;
        } else if (hn == 2) {
          const DPt h0 = hull[0], h1 = hull[1];
          const double dx = h1.x - h0.x, dy = h1.y - h0.y;
          cx = (h0.x + h1.x) / 2; cy = (h0.y + h1.y) / 2;
          w = hypot(dx, dy); h = 0; ang = atan2(dy, dx) * 57.29577951308232;
        }
        merge_finish(snap[pi], snap[pj], sc[pi], sc[pj], cx, cy, w, h, ang, bx[b]);
        const RBox rb = make_rbox(bx[b][0], bx[b][1], bx[b][2], bx[b][3], bx[b][4]);
        rc2[b] = rb.c2; rs2[b] = rb.s2;
      }
      __syncthreads();                                           // (the next pass reuses the hull columns and s_hn)
    }
    __syncthreads();
    // nms_rotated(0.99): stable descending order by rank counting (ties keep the lower index first, as the host's stable
    // sort), then the pairs with IoU >= 0.99 as (earlier, later) sorted positions
#pragma unroll
    for (int r = 0; r < PD_SLOTS; ++r) {
      const int i = tid + r * PD_THREADS;
      if (i < n) {
        const float si = sc[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (sc[j] > si || (sc[j] == si && j < i)) ? 1 : 0;
        order[rank] = (unsigned short)i;
        pos[i] = (unsigned short)rank;
      }
    }
    if (tid == 0) s_hi_n = 0;
    __syncthreads();
    pd_for_pairs(n, bx, queue[tid >> 6], tid, false, [&](int, int) {},
                 [&](int i, int j) {
                   if (rotated_iou_in(rbox_of(bx, i), rbox_of(bx, j), iou_pts) >= 0.99f) {
                     const int e = atomicAdd(&s_hi_n, 1);
                     const int a = min((int)pos[i], (int)pos[j]), c = max((int)pos[i], (int)pos[j]);
                     if (e < hi_cap) pd_ws_store(hi + e, (a << 16) | c);
                   }
                 });
    __syncthreads();
    // greedy suppression as its fixed point: the earliest undecided position has every earlier one decided, so each round
    // decides at least one position (<= n rounds; one or two in practice, none without a listed pair)
    const int n_hi = min(s_hi_n, hi_cap);
#pragma unroll
    for (int r = 0; r < PD_SLOTS; ++r) state[tid + r * PD_THREADS] = n_hi ? 0 : 1;
    __syncthreads();
    for (int round = 0; n_hi && round < n; ++round) {
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r) { mark_kept[tid + r * PD_THREADS] = 0; mark_und[tid + r * PD_THREADS] = 0; }
      if (tid == 0) s_und = 0;
      __syncthreads();
      for (int e = tid; e < n_hi; e += PD_THREADS) {
        const int ent = pd_ws_load(hi + e), a = ent >> 16, c = ent & 0xffff;
        const int sa = state[a];
        if (sa == 1) mark_kept[c] = 1;
        else if (sa == 0) mark_und[c] = 1;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r) {
        const int c = tid + r * PD_THREADS;
        if (c < n && state[c] == 0) {
          if (mark_kept[c]) state[c] = 2;
          else if (!mark_und[c]) state[c] = 1;
          else s_und = 1;
        }
      }
      __syncthreads();
      const int und = s_und;
      __syncthreads();
      if (!und) break;
    }
    // ordered compaction of the survivors (sorted order): read through registers, so no staging arrays
    {
      bool keep[PD_SLOTS];
      int dst[PD_SLOTS];
      float kb[PD_SLOTS][5], ks[PD_SLOTS], kc2[PD_SLOTS], ks2[PD_SLOTS];
      unsigned short ksrc[PD_SLOTS];
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r) {
        const int c = tid + r * PD_THREADS;
        keep[r] = c < n && state[c] == 1;
        const int o = c < n ? order[c] : 0;
#pragma unroll
        for (int e = 0; e < 5; ++e) kb[r][e] = bx[o][e];
        ks[r] = sc[o]; ksrc[r] = src[o]; kc2[r] = rc2[o]; ks2[r] = rs2[o];
      }
      const int m = pd_compact(keep, dst, s_wcnt, tid);
#pragma unroll
      for (int r = 0; r < PD_SLOTS; ++r)
        if (keep[r]) {
          const int d = dst[r];
#pragma unroll
          for (int e = 0; e < 5; ++e) bx[d][e] = kb[r][e];
          sc[d] = ks[r]; src[d] = ksrc[r]; rc2[d] = kc2[r]; rs2[d] = ks2[r];
        }
      if (tid == 0) s_n = m;
    }
    __syncthreads();
  }
  __syncthreads();

  // ---- text decode from the survivors' rows of the per-(box, step) argmax / maximum (text_argmax_kernel), read from global:
  // word score = product of the probabilities before the first stop symbol and at it (or of all T when there is none), text
  // length = characters before the stop; then the thresholds, ordered compaction and the outputs
  const int n_fin = s_n;
  float tscore[PD_SLOTS];
  int tlen[PD_SLOTS], dst[PD_SLOTS];
  bool flag[PD_SLOTS];
#pragma unroll
  for (int r = 0; r < PD_SLOTS; ++r) {
    const int i = tid + r * PD_THREADS;
    tscore[r] = 1.f; tlen[r] = 0; flag[r] = false;
    if (i < n_fin) {
      if (p.do_text) {
        const long g = ((long)n_img * K + src[i]) * p.T;
        bool stopped = false;
        for (int t = 0; t < p.T; ++t) {
          const int bi = p.text_arg[g + t];
          bool take = false;
          if (!stopped) {
            take = true;
            if (bi == p.stop_index) stopped = true; else ++tlen[r];
          }
          if (take) tscore[r] *= p.text_max[g + t];
        }
      }
      flag[r] = (sc[i] >= p.detect_thr) && (!p.do_text || tscore[r] >= p.text_thr);
    }
  }
  const int m_out = pd_compact(flag, dst, s_wcnt, tid);
#pragma unroll
  for (int r = 0; r < PD_SLOTS; ++r)
    if (flag[r]) {
      const int i = tid + r * PD_THREADS;
      const long o = (long)n_img * K + dst[r];
      for (int e = 0; e < 5; ++e) p.out_boxes[o * 5 + e] = bx[i][e];
      p.out_scores[o] = sc[i];
      p.out_src[o] = src[i];
      box_polygon(bx[i], p.out_poly + o * 8);
      p.out_text_score[o] = tscore[r];
      p.out_text_len[o] = tlen[r];
      if (p.do_text) {
        const long g = ((long)n_img * K + src[i]) * p.T;
        for (int t = 0; t < p.T; ++t) p.out_char[o * p.T + t] = p.text_arg[g + t];
      }
    }
  if (tid == 0) p.out_count[n_img] = m_out;
}

extern "C" int64_t glass_postprocess_words_dense_workspace_bytes(int N, int K) {
  if (N <= 0 || K <= 0 || K > PD_KMAX) return 0;
  return (int64_t)N * pd_image_words(K) * 4;
}

extern "C" int glass_postprocess_words_dense(const float* boxes, const float* scores, const int* counts, const int* text_arg,
                                             const float* text_max, const float* scale_xy, int N, int K, int T,
                                             const float* thresholds8_host, int stop_index, float* out_boxes, float* out_scores,
                                             float* out_polygons, int* out_src, int* out_char, float* out_text_score,
                                             int* out_text_len, int* out_count, void* workspace, int64_t workspace_bytes,
                                             glass_stream_t stream) {
  if (N == 0) return GLASS_OK;
  GLASS_CHECK_ARG(N > 0, "glass_postprocess_words_dense: N=%d", N);
  GLASS_CHECK_ARG(K >= 0 && K <= PD_KMAX, "glass_postprocess_words_dense: K=%d (max %d)", K, PD_KMAX);
  GLASS_CHECK_ARG(counts && thresholds8_host && out_count, "glass_postprocess_words_dense: null pointer");
  GLASS_CHECK_ARG(K == 0 || (boxes && scores && out_boxes && out_scores && out_polygons && out_src && out_char &&
                             out_text_score && out_text_len), "glass_postprocess_words_dense: null pointer");
  GLASS_CHECK_ARG((text_arg == nullptr) == (text_max == nullptr), "glass_postprocess_words_dense: text_arg and text_max go together");
  GLASS_CHECK_ARG(!text_arg || (T > 0 && T <= PP_TMAX), "glass_postprocess_words_dense: text needs 0 < T <= %d", PP_TMAX);
  const int64_t need = glass_postprocess_words_dense_workspace_bytes(N, K);
  GLASS_CHECK_ARG(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need),
                  "glass_postprocess_words_dense: workspace of %lld bytes (16-byte aligned), needs %lld", (long long)workspace_bytes,
                  (long long)need);
  PPParams p;
  p.boxes = boxes; p.scores = scores; p.counts = counts; p.text_arg = text_arg; p.text_max = text_max; p.scale_xy = scale_xy;
  p.N = N; p.K = K; p.T = text_arg ? T : 1;
  p.min_box_dim = thresholds8_host[0]; p.valid_score = thresholds8_host[1]; p.detect_thr = thresholds8_host[2];
  p.merge_ioa = thresholds8_host[3]; p.height_ratio = thresholds8_host[4]; p.max_angle_diff = thresholds8_host[5];
  p.minimal_ioa = thresholds8_host[6]; p.text_thr = thresholds8_host[7];
  p.stop_index = stop_index; p.do_text = text_arg ? 1 : 0;
  p.out_boxes = out_boxes; p.out_scores = out_scores; p.out_poly = out_polygons; p.out_src = out_src; p.out_char = out_char;
  p.out_text_score = out_text_score; p.out_text_len = out_text_len; p.out_count = out_count;
  hipLaunchKernelGGL(postprocess_words_dense_kernel, dim3(N), dim3(PD_THREADS), 0, (hipStream_t)stream, p,
                     static_cast<int*>(workspace));
  GLASS_CHECK_LAUNCH("glass_postprocess_words_dense");
  return GLASS_OK;
}
