// Validity and winding of detection rings: one line of sort_detection (reference glass/evaluation/text_evaluator.py:112-137),
// the rule of glass_amd.evaluation.normalize_detection_line, for all rings of a call at once.
//
// Rings are integer rings in the CSR form of rrc_score.hip (pts [P][2], ring_off [n_rings + 1]); |coordinate| <= 2^20 and at
// most 2^20 points per ring, so a coordinate difference fits int32, an orientation determinant is below 2^43 and a shoelace
// sum below 2^62: every product and sum is int64 and exact.  There is no floating point in this file.
//
// Per ring: area2 = sum x_i * y_{i+1} - x_{i+1} * y_i over the closed ring, and verdict 0 (drop: fewer than 3 points, area2
// == 0, or two sides properly cross), 1 (keep: area2 < 0) or 2 (keep reversed: area2 > 0).  Side i is (p_i, p_{(i+1) mod n});
// the pair (i, j) is tested for i + 2 <= j < n except (0, n - 1); sides (p,q) and (r,s) properly cross iff orient(r,s,p),
// orient(r,s,q), orient(p,q,r), orient(p,q,s) are all non-zero, the first two differ in sign and the last two differ in sign.
// Touching, collinear overlap, a repeated vertex and a zero-length side are no crossings.
//
// Work split.  Launch 1, one wave per ring: the lanes stride over the sides, the int64 partial sums are added in an
// xor-shuffle tree (integer addition: the order cannot matter), lane 0 writes area2 and the verdict that n and area2 give.
// Launch 2, the pair tests: a ring is cut into blocks of 64 consecutive sides, B = ceil(n / 64); a task is a block pair
// I <= J of one ring, numbered J * (J + 1) / 2 + I behind task_off[ring] (glass_ring_check_tasks gives the count).  One wave
// serves one task: it finds its ring by binary search in task_off and (I, J) by binary search on the triangular numbers, lane l
// keeps side 64 * I + l in registers, the sides of block J are held one per lane and broadcast one after the other
// (v_readlane, no memory), and every lane tests its side against them under the index rules.  A wave that finds a crossing
// clears the ring's verdict with an integer atomic AND; every writer stores the same 0, so the result does not depend on
// order, grid or neighbours, and two runs are bit-identical.  A long ring is B * (B + 1) / 2 independent tasks, spread over
// the grid.  A task of a ring whose verdict is already 0 is skipped (whatever a racing read returns, the final value is 0).
// No workgroup waits on another; every loop is bounded by a size read once; offsets are clamped to [0, P] as rrc_score.hip
// clamps poly_off, and a task index that does not fit its ring is skipped, so a wrong task_off cannot reach outside pts.
#include "common.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / 64;
constexpr int RC_MAX_BLOCKS = 8192;      // the grid strides over rings / tasks beyond this
constexpr long RC_MAX_POINTS = 1l << 30;

__device__ __forceinline__ long long orient(int ax, int ay, int bx, int by, int cx, int cy) {
  return (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
}

__global__ __launch_bounds__(RC_THREADS) void ring_area_kernel(const int2* __restrict__ pts, long P, const int* __restrict__ ring_off,
                                                               int n_rings, int* __restrict__ verdict,
                                                               long long* __restrict__ area2) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long stride = (long)gridDim.x * RC_WAVES;
  for (long k = (long)blockIdx.x * RC_WAVES + wid; k < n_rings; k += stride) {        // wave-uniform
    const long b = min(max((long)ring_off[k], 0l), P);
    const long n = min(max((long)ring_off[k + 1], b), P) - b;
    long long a2 = 0;
    for (long i = lane; i < n; i += 64) {
      const int2 p = pts[b + i], q = pts[b + (i + 1 == n ? 0 : i + 1)];
      a2 += (long long)p.x * q.y - (long long)q.x * p.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a2 += __shfl_xor(a2, off);
    if (lane == 0) {
      area2[k] = a2;
      verdict[k] = (n < 3 || a2 == 0) ? 0 : (a2 < 0 ? 1 : 2);
    }
  }
}

__global__ __launch_bounds__(RC_THREADS) void ring_cross_kernel(const int2* __restrict__ pts, long P, const int* __restrict__ ring_off,
                                                                int n_rings, const long long* __restrict__ task_off,
                                                                long long n_tasks, int* verdict) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long stride = (long long)gridDim.x * RC_WAVES;
  for (long long t = (long long)blockIdx.x * RC_WAVES + wid; t < n_tasks; t += stride) {   // wave-uniform, as all below but lane
    int lo = 0, hi = n_rings;                                          // the ring: last k with task_off[k] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (task_off[mid] <= t) lo = mid; else hi = mid;
    }
    const int k = lo;
    const long b = min(max((long)ring_off[k], 0l), P);
    const long n = min(max((long)ring_off[k + 1], b), P) - b;
    const long B = (n + 63) >> 6;
    const long long r = t - task_off[k];
    if (n < 3 || r < 0 || r >= (long long)B * (B + 1) / 2) continue;   // not a task of this ring
    if (__builtin_amdgcn_readfirstlane(__atomic_load_n(&verdict[k], __ATOMIC_RELAXED)) == 0) continue;
    long jl = 0, jh = B;                                               // J: last j with j * (j + 1) / 2 <= r
    while (jh - jl > 1) {
      const long jm = (jl + jh) >> 1;
      if ((long long)jm * (jm + 1) / 2 <= r) jl = jm; else jh = jm;
    }
    const long J = jl, I = (long)(r - (long long)J * (J + 1) / 2);     // 0 <= I <= J < B
    const long i = 64 * I + lane, j = 64 * J + lane;
    const bool mine = i < n;
    int2 p = make_int2(0, 0), q = p, u = p, w = p;                     // this lane's side of block I, and of block J
    if (mine) {
      p = pts[b + i];
      q = pts[b + (i + 1 == n ? 0 : i + 1)];
    }
    if (j < n) {
      u = pts[b + j];
      w = pts[b + (j + 1 == n ? 0 : j + 1)];
    }
    const long j0 = 64 * J;
    const int cnt = (int)min(64l, n - j0);                             // sides of block J: 1 .. 64
    bool hit = false;
    for (int m = 0; m < cnt; ++m) {                                    // all lanes are active here: readlane sees every side
      const int rx = __builtin_amdgcn_readlane(u.x, m), ry = __builtin_amdgcn_readlane(u.y, m);
      const int sx = __builtin_amdgcn_readlane(w.x, m), sy = __builtin_amdgcn_readlane(w.y, m);
      const long jj = j0 + m;
      const bool tested = mine && i + 2 <= jj && !(i == 0 && jj == n - 1);
      const long long d1 = orient(rx, ry, sx, sy, p.x, p.y), d2 = orient(rx, ry, sx, sy, q.x, q.y);
      const long long d3 = orient(p.x, p.y, q.x, q.y, rx, ry), d4 = orient(p.x, p.y, q.x, q.y, sx, sy);
      const bool cross = ((d1 > 0) != (d2 > 0)) && ((d3 > 0) != (d4 > 0)) && d1 != 0 && d2 != 0 && d3 != 0 && d4 != 0;
      hit |= tested && cross;
    }
    if (__ballot(hit) != 0 && lane == 0) atomicAnd(&verdict[k], 0);
  }
}

}  // namespace

extern "C" int64_t glass_ring_check_tasks(int n_points_of_ring) {
  if (n_points_of_ring < 3) return 0;
  const int64_t B = ((int64_t)n_points_of_ring + 63) / 64;
  return B * (B + 1) / 2;
}

extern "C" int glass_ring_check(const int* pts, int64_t n_points, const int* ring_off, int n_rings, const int64_t* task_off,
                                int64_t n_tasks, int* verdict, int64_t* area2, glass_stream_t stream) {
  GLASS_CHECK_ARG(n_points >= 0 && n_points <= RC_MAX_POINTS && n_rings >= 0 && n_tasks >= 0,
                  "glass_ring_check: bad sizes n_points=%lld n_rings=%d n_tasks=%lld", (long long)n_points, n_rings,
                  (long long)n_tasks);
  if (n_rings == 0) return GLASS_OK;
  GLASS_CHECK_ARG(verdict && area2, "glass_ring_check: null output");
  hipStream_t st = (hipStream_t)stream;
  if (n_points == 0) {                                                 // every ring is empty: drop, area 0; nothing to launch
    GLASS_CHECK_ARG(n_tasks == 0, "glass_ring_check: %lld tasks but no point", (long long)n_tasks);
    hipError_t e = hipMemsetAsync(verdict, 0, sizeof(int) * (size_t)n_rings, st);
    if (e == hipSuccess) e = hipMemsetAsync(area2, 0, sizeof(int64_t) * (size_t)n_rings, st);
    if (e != hipSuccess) {
      glass_set_error("glass_ring_check: memset failed: %s", hipGetErrorString(e));
      return GLASS_EHIP;
    }
    return GLASS_OK;
  }
  GLASS_CHECK_ARG(pts && ring_off, "glass_ring_check: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)pts & 7) == 0, "glass_ring_check: pts must be 8-byte aligned");
  GLASS_CHECK_ARG(n_tasks == 0 || task_off, "glass_ring_check: %lld tasks need task_off", (long long)n_tasks);
  const int2* p2 = reinterpret_cast<const int2*>(pts);
  hipLaunchKernelGGL(ring_area_kernel, dim3(min(cdiv(n_rings, RC_WAVES), RC_MAX_BLOCKS)), dim3(RC_THREADS), 0, st, p2, (long)n_points,
                     ring_off, n_rings, verdict, reinterpret_cast<long long*>(area2));
  GLASS_CHECK_LAUNCH("glass_ring_check (areas)");
  if (n_tasks > 0) {
    const long long blocks = (n_tasks + RC_WAVES - 1) / RC_WAVES;
    hipLaunchKernelGGL(ring_cross_kernel, dim3((unsigned)(blocks < RC_MAX_BLOCKS ? blocks : RC_MAX_BLOCKS)), dim3(RC_THREADS), 0, st, p2,
                       (long)n_points, ring_off, n_rings, reinterpret_cast<const long long*>(task_off), (long long)n_tasks, verdict);
    GLASS_CHECK_LAUNCH("glass_ring_check");
  }
  return GLASS_OK;
}
