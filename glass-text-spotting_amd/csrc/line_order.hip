// Text lines ordered column by column and cut into blocks (include/glass_hip_feature_layout.h states the contract;
// glass_amd/postprocess/line_order.py:order_lines_host is the same statement in numpy float64).
//
// Four launches, each ordered after the one before by the stream:
//   lo_prep_kernel    one workgroup of 1024 threads per image, thread = line: the page frame by a fixed 1024-slot tree sum,
//                     every valid line's intervals [ulo, uhi], [vlo, vhi] and keys (mv, mu, index), its rank by counting
//                     smaller keys (the invalid lines after the valid ones, in index order), and the bounds of its run of
//                     equal mv.  Everything later is indexed by that rank, so "mv strictly between those of a and b" is the
//                     rank range [run_hi(a), run_lo(b)) of the pair taken in rank order.
//   lo_over_kernel    one wavefront per (image, 64-row block): lane = column rank, a loop over the block's rows, and the ballot
//                     of over(a, b) is the 64-bit row word over[a][b / 64] in the workspace.
//   lo_edges_kernel   same grid: rule 1 from the over bit and the run bounds, rule 2 per pair as
//                     any(over[a] & over[b] & between), at most 16 word operations with the lane's row of `over` and its two
//                     prefix masks in registers; only the words between the two 64-blocks can hold a line between.  The
//                     successor row words and, per row block, each column's count of predecessors go to the workspace.
//   lo_emit_kernel    one workgroup of 1024 threads per image, thread = rank: in-degrees as integer sums over the row blocks,
//                     then L steps, each one integer minimum over (class, rank) - class 0 a ready valid line, 1 an un-ready
//                     valid line (taken only when no line is ready: a forced emission), 2 an invalid line - found by three
//                     ballots per wavefront and sixteen LDS words; every wavefront then reads the one successor word of the
//                     emitted row that covers its 64 lines and decrements.  Then the block cuts, the block boxes by each
//                     run's first thread, and the outputs.
// All arithmetic is float64 without fused multiply-add, there are no float atomics, and nothing here waits for the host.
// Rows beyond the count are never read, and every index taken from memory (a line index, a run bound, the number of valid
// lines) is checked against the count before it is used.
#include "common.h"
#include "glass_hip_feature_layout.h"

#pragma clang fp contract(off)

constexpr int LO_KMAX = GLASS_ORDER_LINES_MAX_K;
constexpr int LO_THREADS = 1024;
constexpr int LO_ROW_WORDS = LO_KMAX / 64;
static_assert(LO_THREADS == LO_KMAX && LO_KMAX % 64 == 0, "one thread per line; the tree sum covers LO_KMAX slots");

typedef unsigned long long lo_u64;

struct LOParams { double min_overlap, max_gap, min_hr; };

// the workspace of one image, in 8-byte words: over | succ | six double arrays by rank, P_U | the int arrays
struct LOLayout {
  long over, succ, dbl, ints, total;
  int W;
};
enum { LO_ULO = 0, LO_UHI, LO_VLO, LO_VHI, LO_MU, LO_H, LO_DBL_ARRAYS };          // double [K] each, then P_U.x, P_U.y
enum { LO_RUNLO = 0, LO_RUNHI, LO_IDX, LO_INT_ARRAYS };                          // int [K] each, then part [W][K], then n_valid

__host__ __device__ inline LOLayout lo_layout(int K) {
  LOLayout y;
  y.W = (K + 63) / 64;
  const long KW = (long)K * y.W;
  y.over = 0;
  y.succ = KW;
  y.dbl = 2 * KW;
  y.ints = y.dbl + (long)LO_DBL_ARRAYS * K + 2;
  const long n_int = (long)LO_INT_ARRAYS * K + KW + 1;
  y.total = (y.ints + (n_int + 1) / 2 + 1) / 2 * 2;                              // a 16-byte multiple
  return y;
}

struct LOLine { double cx, cy, w, h, ux, uy; bool valid; };

// one line from its row: widened exactly, valid iff all five finite and w, h > 0; u = (cos t, -sin t), t = a pi / 180
__device__ inline LOLine lo_load(const float* b) {
  const float f0 = b[0], f1 = b[1], f2 = b[2], f3 = b[3], f4 = b[4];
  LOLine q;
  q.valid = isfinite(f0) && isfinite(f1) && isfinite(f2) && isfinite(f3) && isfinite(f4) && f2 > 0.f && f3 > 0.f;
  q.cx = (double)f0; q.cy = (double)f1; q.w = (double)f2; q.h = (double)f3;
  q.ux = 1.0; q.uy = 0.0;
  if (q.valid) {
    const double t = (double)f4 * 3.14159265358979323846 / 180.0;
    q.ux = cos(t); q.uy = -sin(t);
  }
  return q;
}

__device__ __forceinline__ int lo_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the bits of word k that stand for ranks below x
__device__ __forceinline__ lo_u64 lo_below(int x, int k) {
  const int d = x - 64 * k;
  return d <= 0 ? 0ull : (d >= 64 ? ~0ull : ((1ull << d) - 1ull));
}

// ------------------------------------------------------------------------------------------------ frame, intervals, ranks
__global__ __launch_bounds__(LO_THREADS) void lo_prep_kernel(const float* __restrict__ boxes, const int* __restrict__ count, int K,
                                                             lo_u64* __restrict__ ws) {
  __shared__ double s_dx[LO_KMAX], s_dy[LO_KMAX], s_sw[LO_KMAX];           // the tree sums
  __shared__ double s_mv[LO_KMAX], s_mu[LO_KMAX];
  __shared__ unsigned char s_valid[LO_KMAX];
  const int img = blockIdx.x, t = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  const LOLayout y = lo_layout(K);
  lo_u64* base = ws + (long)img * y.total;
  double* dbl = reinterpret_cast<double*>(base + y.dbl);
  int* ints = reinterpret_cast<int*>(base + y.ints);

  LOLine q{0., 0., 0., 0., 1., 0., false};
  if (t < n) q = lo_load(boxes + ((long)img * K + t) * 5);
  s_dx[t] = q.valid ? q.w * q.ux : 0.0;
  s_dy[t] = q.valid ? q.w * q.uy : 0.0;
  s_sw[t] = q.valid ? q.w : 0.0;
  s_valid[t] = q.valid ? 1 : 0;
  __syncthreads();
  for (int stride = LO_KMAX / 2; stride > 0; stride >>= 1) {
    if (t < stride) { s_dx[t] += s_dx[t + stride]; s_dy[t] += s_dy[t + stride]; s_sw[t] += s_sw[t + stride]; }
    __syncthreads();
  }
  double PUx = 1.0, PUy = 0.0;
  {
    const double Dx = s_dx[0], Dy = s_dy[0], Sw = s_sw[0];
    const double nrm = sqrt(Dx * Dx + Dy * Dy);
    if (nrm > 1e-12 * Sw) { PUx = Dx / nrm; PUy = Dy / nrm; }
  }
  const double PVx = -PUy, PVy = PUx;

  double ulo = 0, uhi = 0, vlo = 0, vhi = 0, mu = 0, mv = 0;
  if (q.valid) {
    const double hw = q.w / 2, hh = q.h / 2;
    const double ax = hw * q.ux, ay = hw * q.uy, bx = hh * -q.uy, by = hh * q.ux;       // (w / 2) u and (h / 2) v
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double su = (c & 1) ? -1.0 : 1.0, sv = (c & 2) ? -1.0 : 1.0;
      const double px = q.cx + su * ax + sv * bx, py = q.cy + su * ay + sv * by;
      const double pu = px * PUx + py * PUy, pv = px * PVx + py * PVy;
      if (c == 0) { ulo = uhi = pu; vlo = vhi = pv; }
      else { ulo = fmin(ulo, pu); uhi = fmax(uhi, pu); vlo = fmin(vlo, pv); vhi = fmax(vhi, pv); }
    }
    mu = q.cx * PUx + q.cy * PUy;
    mv = q.cx * PVx + q.cy * PVy;
  }
  s_mv[t] = mv; s_mu[t] = mu;
  const int n_valid = __syncthreads_count(q.valid);

  if (t < n) {
    int r = 0, lo = 0, hi = 0;
    if (q.valid) {
#pragma unroll 8
      for (int j = 0; j < n; ++j) {
        const bool vj = s_valid[j] != 0;
        const double mvj = s_mv[j], muj = s_mu[j];
        lo += (vj && mvj < mv) ? 1 : 0;
        hi += (vj && mvj <= mv) ? 1 : 0;
        r += (vj && (mvj < mv || (mvj == mv && (muj < mu || (muj == mu && j < t))))) ? 1 : 0;
      }
    } else {
      r = n_valid;
      for (int j = 0; j < t; ++j) r += s_valid[j] ? 0 : 1;
      lo = r; hi = r + 1;
    }
    dbl[LO_ULO * K + r] = ulo; dbl[LO_UHI * K + r] = uhi; dbl[LO_VLO * K + r] = vlo; dbl[LO_VHI * K + r] = vhi;
    dbl[LO_MU * K + r] = mu; dbl[LO_H * K + r] = q.h;
    ints[LO_RUNLO * K + r] = lo; ints[LO_RUNHI * K + r] = hi; ints[LO_IDX * K + r] = t;
  }
  if (t == 0) {
    dbl[LO_DBL_ARRAYS * K] = PUx; dbl[LO_DBL_ARRAYS * K + 1] = PUy;
    ints[LO_INT_ARRAYS * K + (long)K * y.W] = n_valid;
  }
}

// ------------------------------------------------------------------------------------------------ the over relation
__global__ __launch_bounds__(64) void lo_over_kernel(const int* __restrict__ count, int K, double min_overlap, lo_u64* __restrict__ ws) {
  __shared__ double s_ulo[LO_KMAX], s_uhi[LO_KMAX];
  const int img = blockIdx.y, rb = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  const LOLayout y = lo_layout(K);
  lo_u64* base = ws + (long)img * y.total;
  const double* dbl = reinterpret_cast<const double*>(base + y.dbl);
  const int* ints = reinterpret_cast<const int*>(base + y.ints);
  const int V = lo_clamp(ints[LO_INT_ARRAYS * K + (long)K * y.W], 0, n);          // the valid lines are the ranks below V
  if (rb * 64 >= V) return;
  for (int j = lane; j < V; j += 64) { s_ulo[j] = dbl[LO_ULO * K + j]; s_uhi[j] = dbl[LO_UHI * K + j]; }
  __syncthreads();
  lo_u64* over = base + y.over;
  const int nb = (V + 63) / 64, rows = min(64, V - rb * 64);
  for (int jb = 0; jb < nb; ++jb) {
    const int j = jb * 64 + lane;
    const bool jv = j < V;
    const double loj = s_ulo[jv ? j : 0], hij = s_uhi[jv ? j : 0];
    const double lenj = hij - loj;
    lo_u64 mine = 0ull;
    for (int ii = 0; ii < rows; ++ii) {
      const int i = rb * 64 + ii;                                   // (wavefront-uniform: the reads of line i are broadcasts)
      const double loi = s_ulo[i], hii = s_uhi[i];
      const bool ov = jv && i != j && fmin(hii, hij) - fmax(loi, loj) > min_overlap * fmin(hii - loi, lenj);
      const lo_u64 m = __ballot(ov);
      if (lane == ii) mine = m;
    }
    if (lane < rows) over[(long)(rb * 64 + lane) * y.W + jb] = mine;
  }
}

// ------------------------------------------------------------------------------------------------ the two rules
__global__ __launch_bounds__(64) void lo_edges_kernel(const int* __restrict__ count, int K, lo_u64* __restrict__ ws) {
  __shared__ double s_mu[LO_KMAX];
  __shared__ int s_runlo[LO_KMAX], s_runhi[LO_KMAX];
  const int img = blockIdx.y, rb = blockIdx.x, lane = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  const LOLayout y = lo_layout(K);
  lo_u64* base = ws + (long)img * y.total;
  const double* dbl = reinterpret_cast<const double*>(base + y.dbl);
  int* ints = reinterpret_cast<int*>(base + y.ints);
  const int V = lo_clamp(ints[LO_INT_ARRAYS * K + (long)K * y.W], 0, n);
  if (rb * 64 >= V) return;
  for (int j = lane; j < V; j += 64) {
    s_mu[j] = dbl[LO_MU * K + j];
    s_runlo[j] = lo_clamp(ints[LO_RUNLO * K + j], 0, V);
    s_runhi[j] = lo_clamp(ints[LO_RUNHI * K + j], 0, V);
  }
  __syncthreads();
  const lo_u64* over = base + y.over;
  lo_u64* succ = base + y.succ;
  int* part = ints + LO_INT_ARRAYS * K;                             // part[rb][b]: predecessors of b among the rows of block rb
  const int W = y.W, nb = (V + 63) / 64, rows = min(64, V - rb * 64);
  for (int jb = 0; jb < nb; ++jb) {
    const int b = jb * 64 + lane;
    const bool bv = b < V;
    const int bs = bv ? b : 0;
    const double mub = s_mu[bs];
    const int lob = s_runlo[bs], hib = s_runhi[bs];
    // a line between a and b in mv has its rank between theirs, so only the words klo .. khi can hold one
    const int klo = min(rb, jb), khi = max(rb, jb);
    lo_u64 ovb[LO_ROW_WORDS], below_lob[LO_ROW_WORDS], below_hib[LO_ROW_WORDS];
#pragma unroll
    for (int k = 0; k < LO_ROW_WORDS; ++k) {
      ovb[k] = (bv && k >= klo && k <= khi) ? over[(long)b * W + k] : 0ull;
      below_lob[k] = lo_below(lob, k);
      below_hib[k] = lo_below(hib, k);
    }
    lo_u64 mine = 0ull;
    int cnt = 0;
    for (int ii = 0; ii < rows; ++ii) {
      const int a = rb * 64 + ii;                                   // (wavefront-uniform)
      const lo_u64* rowa = over + (long)a * W;
      const int loa = __builtin_amdgcn_readfirstlane(s_runlo[a]), hia = __builtin_amdgcn_readfirstlane(s_runhi[a]);
      const double mua = s_mu[a];
      const bool ovab = (rowa[jb] >> lane) & 1ull;
      bool edge = false;
      if (bv && a != b) {
        if (ovab) edge = loa < lob;                                 // rule 1: mv_a < mv_b
        else if (mua < mub) {                                       // rule 2
          const bool a_first = a < b;                               // between = [run_hi(first), run_lo(second))
          lo_u64 any = 0ull;
#pragma unroll
          for (int k = 0; k < LO_ROW_WORDS; ++k) {
            if (k >= klo && k <= khi) {
              const lo_u64 between = a_first ? (below_lob[k] & ~lo_below(hia, k)) : (lo_below(loa, k) & ~below_hib[k]);
              any |= rowa[k] & ovb[k] & between;
            }
          }
          edge = any == 0ull;
        }
      }
      const lo_u64 m = __ballot(edge);
      if (lane == ii) mine = m;
      cnt += edge ? 1 : 0;
    }
    if (lane < rows) succ[(long)(rb * 64 + lane) * W + jb] = mine;
    if (bv) part[(long)rb * K + b] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ emission, blocks, outputs
// exclusive prefix sum of v over the workgroup's threads; `total` is the sum.  s_w: 16 ints of LDS, free again on return.
__device__ __forceinline__ int lo_scan(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < LO_THREADS / 64; ++w) {
    const int x = s_w[w];
    before += w < wave ? x : 0;
    all += x;
  }
  __syncthreads();
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(LO_THREADS) void lo_emit_kernel(const float* __restrict__ boxes, const int* __restrict__ count,
                                                             const int* __restrict__ line_start, int K, LOParams p,
                                                             const lo_u64* __restrict__ ws, int* __restrict__ page_rank,
                                                             int* __restrict__ page_order, int* __restrict__ block_id,
                                                             int* __restrict__ block_start, float* __restrict__ block_boxes,
                                                             int* __restrict__ block_count, int* __restrict__ forced_out,
                                                             int* __restrict__ line_first) {
  __shared__ double s_ulo[LO_KMAX], s_uhi[LO_KMAX], s_vlo[LO_KMAX], s_vhi[LO_KMAX], s_h[LO_KMAX];     // 40 KB, by rank
  __shared__ int s_runlo[LO_KMAX], s_idx[LO_KMAX], s_at[LO_KMAX];          // s_at[position] = rank
  __shared__ unsigned char s_cut[LO_KMAX];                                 // by position: a block starts here
  __shared__ int s_wmin[2][LO_THREADS / 64], s_scan[LO_THREADS / 64];
  const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int L = min(max(count[img], 0), K);
  const LOLayout y = lo_layout(K);
  const lo_u64* base = ws + (long)img * y.total;
  const double* dbl = reinterpret_cast<const double*>(base + y.dbl);
  const int* ints = reinterpret_cast<const int*>(base + y.ints);
  const lo_u64* over = base + y.over;
  const lo_u64* succ = base + y.succ;
  const int* part = ints + LO_INT_ARRAYS * K;
  const int W = y.W;
  const int V = lo_clamp(ints[LO_INT_ARRAYS * K + (long)K * W], 0, L);
  const int nb = (V + 63) / 64;
  const double PUx = dbl[LO_DBL_ARRAYS * K], PUy = dbl[LO_DBL_ARRAYS * K + 1];
  const double PVx = -PUy, PVy = PUx;
  const long o = (long)img * K;

  // ---- the line of rank t; its in-degree
  int idx = 0, indeg = 0;
  if (t < L) {
    s_ulo[t] = dbl[LO_ULO * K + t]; s_uhi[t] = dbl[LO_UHI * K + t]; s_vlo[t] = dbl[LO_VLO * K + t]; s_vhi[t] = dbl[LO_VHI * K + t];
    s_h[t] = dbl[LO_H * K + t];
    s_runlo[t] = ints[LO_RUNLO * K + t];
    idx = lo_clamp(ints[LO_IDX * K + t], 0, L - 1);
    s_idx[t] = idx;
    if (t < V)
      for (int rb = 0; rb < nb; ++rb) indeg += part[(long)rb * K + t];
  }
  const bool valid = t < V;

  // ---- the emission: L steps, each the minimum of (class, rank) over the lines not yet emitted
  bool emitted = t >= L;
  int pos = 0, forced = 0;
  for (int s = 0; s < L; ++s) {
    const int cls = emitted ? 3 : (!valid ? 2 : (indeg > 0 ? 1 : 0));
    const lo_u64 b0 = __ballot(cls == 0), b1 = __ballot(cls == 1), b2 = __ballot(cls == 2);
    if (lane == 0) {
      int code = 0x7fffffff;
      if (b0) code = (0 << 10) | (wave * 64 + __ffsll((long long)b0) - 1);
      else if (b1) code = (1 << 10) | (wave * 64 + __ffsll((long long)b1) - 1);
      else if (b2) code = (2 << 10) | (wave * 64 + __ffsll((long long)b2) - 1);
      s_wmin[s & 1][wave] = code;
    }
    __syncthreads();                       // (one barrier a step: the buffer written two steps on was read before the next barrier)
    int best = 0x7fffffff;
#pragma unroll
    for (int w = 0; w < LO_THREADS / 64; ++w) best = min(best, s_wmin[s & 1][w]);
    const int e = best & 1023, ecls = best >> 10;          // (best is a code of one of this workgroup's un-emitted lines: s < L)
    if (t == e) { emitted = true; pos = s; }
    forced += ecls == 1 ? 1 : 0;
    if (ecls < 2 && wave < nb) {
      const lo_u64 m = succ[(long)e * W + wave];
      indeg -= (valid && ((m >> lane) & 1ull)) ? 1 : 0;
    }
  }
  if (t < L) s_at[pos] = t;
  __syncthreads();

  // ---- block cuts, by position
  bool cut = false;
  int r = 0;
  if (t < L) {
    r = s_at[t];
    cut = true;
    if (t > 0) {
      const int pr = s_at[t - 1];
      if (pr < V && r < V) {
        const bool ov = (over[(long)pr * W + (r >> 6)] >> (r & 63)) & 1ull;
        const double hp = s_h[pr], hq = s_h[r];
        const double H = fmax(hp, hq), hmin = fmin(hp, hq);
        cut = !(ov && s_runlo[pr] < s_runlo[r] && s_vlo[r] - s_vhi[pr] <= p.max_gap * H && hmin >= p.min_hr * H);
      }
    }
  }
  s_cut[t] = cut ? 1 : 0;
  int n_blocks = 0;
  const int cuts_before = lo_scan(cut ? 1 : 0, s_scan, n_blocks);           // (its barriers publish s_cut)
  const int bid = cuts_before + (cut ? 1 : 0) - 1;                          // the block of position t

  // ---- words ahead of the line, by position
  if (line_start != nullptr) {
    int size = 0;
    if (t < L) {
      const int* ls = line_start + (long)img * (K + 1);
      const int i = s_idx[r];
      const int a = ls[i], b = ls[i + 1];
      size = (a >= 0 && a <= b && b <= K) ? b - a : 0;
    }
    int all = 0;
    const int ahead = lo_scan(size, s_scan, all);
    if (t < L) line_first[o + s_idx[r]] = ahead;
    else if (t < K) line_first[o + t] = -1;
  }

  // ---- the outputs: by line index, by position, by block
  if (t < L) {
    const int i = s_idx[r];
    page_rank[o + i] = t;
    page_order[o + t] = i;
    block_id[o + i] = bid;
    if (cut) {
      block_start[(long)img * (K + 1) + bid] = t;
      float* bb = block_boxes + (o + bid) * 5;
      if (r < V) {
        double umin = s_ulo[r], umax = s_uhi[r], vmin = s_vlo[r], vmax = s_vhi[r];
        for (int q = t + 1; q < L && !s_cut[q]; ++q) {
          const int rq = s_at[q];
          umin = fmin(umin, s_ulo[rq]); umax = fmax(umax, s_uhi[rq]); vmin = fmin(vmin, s_vlo[rq]); vmax = fmax(vmax, s_vhi[rq]);
        }
        const double cu = (umin + umax) / 2, cv = (vmin + vmax) / 2;
        bb[0] = (float)(cu * PUx + cv * PVx); bb[1] = (float)(cu * PUy + cv * PVy);
        bb[2] = (float)(umax - umin); bb[3] = (float)(vmax - vmin);
        bb[4] = (float)(atan2(-PUy, PUx) * 180.0 / 3.14159265358979323846);
      } else {
        const unsigned* src = reinterpret_cast<const unsigned*>(boxes + (o + i) * 5);
        unsigned* dst = reinterpret_cast<unsigned*>(bb);
        for (int e = 0; e < 5; ++e) dst[e] = src[e];
      }
    }
  } else if (t < K) {
    page_rank[o + t] = -1; page_order[o + t] = -1; block_id[o + t] = -1;
  }
  if (t >= n_blocks && t < K)
    for (int e = 0; e < 5; ++e) block_boxes[(o + t) * 5 + e] = 0.f;
  for (int e = n_blocks + t; e <= K; e += LO_THREADS) block_start[(long)img * (K + 1) + e] = L;
  if (t == 0) { block_count[img] = n_blocks; forced_out[img] = forced; }
}

extern "C" int64_t glass_order_lines_workspace_bytes(int N, int K) {
  if (N < 0 || K < 0 || K > LO_KMAX) return -1;
  return (int64_t)N * lo_layout(K).total * 8;
}

extern "C" int glass_order_lines(const float* line_boxes, const int* line_count, const int* line_start, int N, int K,
                                 const double* params3_host, int* page_rank, int* page_order, int* block_id, int* block_start,
                                 float* block_boxes, int* block_count, int* forced, int* line_first, void* workspace,
                                 int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(N >= 0, "glass_order_lines: N=%d", N);
  GLASS_CHECK_ARG(K >= 0 && K <= LO_KMAX, "glass_order_lines: K=%d (max %d)", K, LO_KMAX);
  GLASS_CHECK_ARG(params3_host, "glass_order_lines: null parameters");
  LOParams p{params3_host[0], params3_host[1], params3_host[2]};
  GLASS_CHECK_ARG(p.min_overlap >= 0 && p.min_overlap < 1, "glass_order_lines: min_overlap=%g (0 <= . < 1)", p.min_overlap);
  GLASS_CHECK_ARG(p.max_gap >= 0 && p.max_gap <= 1.7e308, "glass_order_lines: block_max_gap=%g (finite, >= 0)", p.max_gap);
  GLASS_CHECK_ARG(p.min_hr >= 0 && p.min_hr <= 1, "glass_order_lines: block_min_height_ratio=%g (0..1)", p.min_hr);
  GLASS_CHECK_ARG(K == 0 || (line_start == nullptr) == (line_first == nullptr), "glass_order_lines: line_start and line_first go together");
  if (N == 0) return GLASS_OK;
  GLASS_CHECK_ARG(line_count && block_start && block_count && forced, "glass_order_lines: null pointer");
  GLASS_CHECK_ARG(K == 0 || (line_boxes && page_rank && page_order && block_id && block_boxes), "glass_order_lines: null pointer");
  const int64_t need = glass_order_lines_workspace_bytes(N, K);
  GLASS_CHECK_ARG(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need),
                  "glass_order_lines: workspace of %lld bytes (16-byte aligned), needs %lld", (long long)workspace_bytes,
                  (long long)need);
  lo_u64* ws = static_cast<lo_u64*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (K > 0) {
    const int W = lo_layout(K).W;
    hipLaunchKernelGGL(lo_prep_kernel, dim3(N), dim3(LO_THREADS), 0, st, line_boxes, line_count, K, ws);
    GLASS_CHECK_LAUNCH("glass_order_lines (prep)");
    hipLaunchKernelGGL(lo_over_kernel, dim3(W, N), dim3(64), 0, st, line_count, K, p.min_overlap, ws);
    GLASS_CHECK_LAUNCH("glass_order_lines (over)");
    hipLaunchKernelGGL(lo_edges_kernel, dim3(W, N), dim3(64), 0, st, line_count, K, ws);
    GLASS_CHECK_LAUNCH("glass_order_lines (edges)");
  }
  hipLaunchKernelGGL(lo_emit_kernel, dim3(N), dim3(LO_THREADS), 0, st, line_boxes, line_count, line_start, K, p,
                     static_cast<const lo_u64*>(ws), page_rank, page_order, block_id, block_start, block_boxes, block_count, forced,
                     line_first);
  GLASS_CHECK_LAUNCH("glass_order_lines (emit)");
  return GLASS_OK;
}
