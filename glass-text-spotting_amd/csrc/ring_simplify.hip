// Exact Douglas-Peucker simplification of traced rings (include/glass_hip_feature_simplify.h has the contract; the statement
// is glass_amd/evaluation/ring_simplify.py simplify_ring, which this file equals vertex for vertex).
//
// Rings come in the CSR form the tracers leave (xy [V][2], ring_off [R + 1]), |coordinate| <= 2^20.  A coordinate
// difference is below 2^22 in magnitude, L = d.d and |w|^2 below 2^44, a cross product below 2^44: `num` is always a product
// X * Y of two unsigned 64-bit values (|w|^2 * L, |p - b|^2 * L, |c| * |c|), kept as the pair (high, low) of the exact
// 128-bit product.  16 * num < 2^92 shifts without loss, q4^2 * L < 2^68.  There is no floating point in this file.
//
// Work split.  One workgroup is one wavefront and owns one ring at a time (the grid strides over the rings).  It stages the
// ring in LDS if it has at most GLASS_RING_SIMPLIFY_LDS_POINTS points and otherwise reads global memory through the same
// accessor.  For a chain (lo, hi) the lanes stride over the interior, each keeps its best (num, earliest position), and an
// xor-shuffle tree takes the maximum under the total order "larger num, then smaller position": every lane ends with the same
// triple whatever the tree's shape.  Pending chains wait on a stack held one entry per lane (entry k in lane k's registers,
// read with a shuffle): the loop continues with the shorter half and pushes the longer, so an entry is pushed only when the
// current chain has at most half the length of the entry below it, and 2^31 points need at most 32 entries of the 64.
// A keep flag is written by the lane that cleared it (lane = position mod 64), so its two stores are ordered by the program
// order of one thread.  Kept counts go to the workspace; a one-workgroup running sum turns them into out_off; the write
// kernel compacts each ring with ballots.  Every loop is bounded by a size read once, offsets are validated before they index.
#include <climits>

#include "common.h"
#include "glass_hip_feature_simplify.h"

namespace {

constexpr int RS_LDS_POINTS = GLASS_RING_SIMPLIFY_LDS_POINTS;
constexpr int RS_MAX_COORD = 1 << 20;
constexpr int RS_MAX_Q4 = 4096;
constexpr int RS_STACK = 64;             // one entry per lane
constexpr int RS_MAX_BLOCKS = 1 << 16;   // the grid strides over the rings beyond this
constexpr int RS_SCAN_THREADS = 256;
enum { RS_OK = 0, RS_BAD_COORD = 1, RS_BAD_OFFSET = 2, RS_STACK_FULL = 3 };

typedef unsigned long long u64;

struct Best {
  u64 hi, lo;   // num, the exact 128-bit product
  int pos;      // INT_MAX: no candidate
};

__device__ __forceinline__ bool rs_better(const Best& a, const Best& b) {
  return a.hi > b.hi || (a.hi == b.hi && (a.lo > b.lo || (a.lo == b.lo && a.pos < b.pos)));
}

__device__ __forceinline__ Best rs_wave_best(Best v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best o;
    o.hi = __shfl_xor(v.hi, off);
    o.lo = __shfl_xor(v.lo, off);
    o.pos = __shfl_xor(v.pos, off);
    if (rs_better(o, v)) v = o;
  }
  return v;
}

// num of p against the chord (a, b) as the factors X * Y; *Leff = L, or 1 for a == b
__device__ __forceinline__ void rs_num(int2 a, int2 b, int2 p, u64* hi, u64* lo) {
  const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
  const long long wx = (long long)p.x - a.x, wy = (long long)p.y - a.y;
  const long long L = dx * dx + dy * dy, t = wx * dx + wy * dy;
  u64 X, Y;
  if (L == 0) {
    X = (u64)(wx * wx + wy * wy);
    Y = 1;
  } else if (t <= 0) {
    X = (u64)(wx * wx + wy * wy);
    Y = (u64)L;
  } else if (t >= L) {
    const long long ux = (long long)p.x - b.x, uy = (long long)p.y - b.y;
    X = (u64)(ux * ux + uy * uy);
    Y = (u64)L;
  } else {
    const long long c = dx * wy - dy * wx;
    X = Y = (u64)(c < 0 ? -c : c);
  }
  *hi = __umul64hi(X, Y);
  *lo = X * Y;
}

// the ring's points: LDS if staged, else global memory; position n is v[0] again
struct Ring {
  const int2* g;
  const int2* sh;
  bool staged;
  int n;
  __device__ __forceinline__ int2 at(int i) const {
    if (i == n) i = 0;
    return staged ? sh[i] : g[i];
  }
};

// best (num, earliest position) of positions first .. last - 1 against the chord (a, b); the same value in every lane
__device__ __forceinline__ Best rs_farthest(const Ring& R, int2 a, int2 b, int first, int last, int lane) {
  Best v;
  v.hi = v.lo = 0;
  v.pos = INT_MAX;
  for (long long i = (long long)first + lane; i < last; i += 64) {
    Best c;
    rs_num(a, b, R.at((int)i), &c.hi, &c.lo);
    c.pos = (int)i;
    if (rs_better(c, v)) v = c;     // ascending i: an equal num never replaces an earlier position
  }
  return rs_wave_best(v);
}

// 16 * num > q4sq * L, all 128-bit
__device__ __forceinline__ bool rs_farther(const Best& v, u64 q4sq, int2 a, int2 b) {
  const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
  u64 L = (u64)(dx * dx + dy * dy);
  if (L == 0) L = 1;
  const u64 lhs_hi = (v.hi << 4) | (v.lo >> 60), lhs_lo = v.lo << 4;
  const u64 rhs_hi = __umul64hi(q4sq, L), rhs_lo = q4sq * L;
  return lhs_hi > rhs_hi || (lhs_hi == rhs_hi && lhs_lo > rhs_lo);
}

__global__ __launch_bounds__(64) void rs_mark_kernel(const int2* __restrict__ xy, long long V, const int* __restrict__ ring_off,
                                                     int n_rings, int q4, unsigned char* __restrict__ flags,
                                                     int* __restrict__ counts, int* status) {
  __shared__ int2 sh[RS_LDS_POINTS];
  const int lane = threadIdx.x;
  const u64 q4sq = (u64)q4 * (u64)q4;
  for (int r = blockIdx.x; r < n_rings; r += gridDim.x) {                // wave-uniform, as everything below but `lane`
    const long long b = ring_off[r], e = ring_off[r + 1];
    if (b < 0 || e < b || e > V) {
      if (lane == 0) {
        atomicMax(status, (int)RS_BAD_OFFSET);
        counts[r] = 0;
      }
      continue;
    }
    const int m = (int)(e - b);                                          // V < 2^31
    if (m == 0) {
      if (lane == 0) counts[r] = 0;
      continue;
    }
    Ring R;
    R.g = xy + b;
    R.sh = sh;
    R.staged = m <= RS_LDS_POINTS;
    unsigned char* f = flags + b;
    __syncthreads();                                                     // the previous ring's reads of sh are done
    bool bad = false;
    for (int i = lane; i < m; i += 64) {
      const int2 p = R.g[i];
      bad |= p.x > RS_MAX_COORD || p.x < -RS_MAX_COORD || p.y > RS_MAX_COORD || p.y < -RS_MAX_COORD;
      if (R.staged) sh[i] = p;
    }
    __syncthreads();
    if (__ballot(bad) != 0ull) {
      if (lane == 0) {
        atomicMax(status, (int)RS_BAD_COORD);
        counts[r] = 0;
      }
      continue;
    }
    const int2 A = R.g[0], last = R.g[m - 1];
    const bool closed = m >= 2 && last.x == A.x && last.y == A.y;
    const int n = closed ? m - 1 : m;
    R.n = n;
    // B: the vertex farthest from A, lowest index on a tie (num = |v - A|^2 as a 64-bit value)
    Best far;
    far.hi = far.lo = 0;
    far.pos = INT_MAX;
    if (n > 3) {
      for (int i = lane; i < n; i += 64) {
        const int2 p = R.at(i);
        const long long wx = (long long)p.x - A.x, wy = (long long)p.y - A.y;
        Best c;
        c.hi = 0;
        c.lo = (u64)(wx * wx + wy * wy);
        c.pos = i;
        if (rs_better(c, far)) far = c;
      }
      far = rs_wave_best(far);
    }
    if (n <= 3 || far.lo == 0) {                                         // short, or every vertex equals A: unchanged
      for (int i = lane; i < m; i += 64) f[i] = 1;
      if (lane == 0) counts[r] = m;
      continue;
    }
    const int B = far.pos;                                               // 1 .. n - 1
    for (int i = lane; i < m; i += 64) f[i] = (i == 0 || i == B || i == n) ? 1 : 0;     // i == n: the closing duplicate
    const int2 PB = R.at(B);
    int kept = 2, sp = 0, slo = 0, shi = 0;                              // stack entry k lives in lane k
    bool overflow = false;
    // the two chains: (0, B) first on the stack, (B, n) the current one
    if (B > 1) {
      if (lane == sp) {
        slo = 0;
        shi = B;
      }
      ++sp;
    }
    int lo = B, hi = n;
    for (;;) {
      while (hi - lo >= 2) {
        const int2 a = R.at(lo), c = R.at(hi);
        const Best v = rs_farthest(R, a, c, lo + 1, hi, lane);
        if (!rs_farther(v, q4sq, a, c)) break;                           // the whole interior is dropped
        const int mid = v.pos;
        if ((mid & 63) == lane) f[mid] = 1;
        ++kept;
        int plo, phi;                                                    // push the longer half, go on with the shorter
        if (mid - lo <= hi - mid) {
          plo = mid;
          phi = hi;
          hi = mid;
        } else {
          plo = lo;
          phi = mid;
          lo = mid;
        }
        if (phi - plo >= 2) {
          if (sp >= RS_STACK) {
            overflow = true;
            break;
          }
          if (lane == sp) {
            slo = plo;
            shi = phi;
          }
          ++sp;
        }
      }
      if (sp == 0 || overflow) break;
      --sp;
      lo = __shfl(slo, sp);
      hi = __shfl(shi, sp);
    }
    if (overflow) {
      if (lane == 0) {
        atomicMax(status, (int)RS_STACK_FULL);
        counts[r] = 0;
      }
      continue;
    }
    if (kept == 2) {                                                     // never lose a ring: a third vertex off the chord (A, B)
      const Best v = rs_farthest(R, A, PB, 0, n, lane);
      if ((v.hi | v.lo) != 0) {
        if ((v.pos & 63) == lane) f[v.pos] = 1;
        ++kept;
      }
    }
    if (lane == 0) counts[r] = kept + (closed ? 1 : 0);
  }
}

// out_off = running sum of counts, or all zeros after a failed mark
__global__ __launch_bounds__(RS_SCAN_THREADS) void rs_offsets_kernel(const int* __restrict__ counts, int n_rings,
                                                                     int* __restrict__ out_off, const int* __restrict__ status) {
  __shared__ long long part[RS_SCAN_THREADS];
  const int tid = threadIdx.x;
  if (*status != RS_OK) {
    for (int r = tid; r <= n_rings; r += RS_SCAN_THREADS) out_off[r] = 0;
    return;
  }
  const int per = (n_rings + RS_SCAN_THREADS - 1) / RS_SCAN_THREADS;
  const int b = (int)min((long long)n_rings, (long long)tid * per), e = (int)min((long long)n_rings, (long long)b + per);
  long long s = 0;
  for (int k = b; k < e; ++k) s += counts[k];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int k = 0; k < RS_SCAN_THREADS; ++k) {
      const long long v = part[k];
      part[k] = run;
      run += v;
    }
    out_off[n_rings] = (int)run;                                         // at most V < 2^31: the kept points are a subset
  }
  __syncthreads();
  s = part[tid];
  for (int k = b; k < e; ++k) {
    out_off[k] = (int)s;
    s += counts[k];
  }
}

__global__ __launch_bounds__(64) void rs_write_kernel(const int2* __restrict__ xy, long long V, const int* __restrict__ ring_off,
                                                      int n_rings, const unsigned char* __restrict__ flags,
                                                      const int* __restrict__ out_off, int2* __restrict__ out, long long n_out) {
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < n_rings; r += gridDim.x) {
    const long long b = ring_off[r], e = ring_off[r + 1];
    if (b < 0 || e < b || e > V) continue;
    const long long ob = out_off[r], oe = min((long long)out_off[r + 1], n_out);
    if (ob < 0) continue;
    const long long m = e - b;
    long long run = ob;
    for (long long base = 0; base < m; base += 64) {
      const long long i = base + lane;
      const bool keep = i < m && flags[b + i] != 0;
      const u64 bal = __ballot(keep);
      const long long o = run + __popcll(bal & ((1ull << lane) - 1ull));
      if (keep && o < oe) out[o] = xy[b + i];
      run += __popcll(bal);
    }
  }
}

int64_t rs_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

// workspace: counts int32 [n_rings] | flags uint8 [n_points]
extern "C" int64_t glass_ring_simplify_workspace_bytes(int64_t n_points, int n_rings) {
  if (n_points < 0 || n_points > INT_MAX || n_rings < 0) return GLASS_EINVAL;
  return rs_align16((int64_t)n_rings * 4) + rs_align16(n_points);
}

extern "C" int glass_ring_simplify_mark(const int* xy, int64_t n_points, const int* ring_off, int n_rings, int q4, void* workspace,
                                        int64_t workspace_bytes, int* out_off, int* status, glass_stream_t stream) {
  GLASS_CHECK_ARG(n_points >= 0 && n_points <= INT_MAX && n_rings >= 0, "glass_ring_simplify_mark: bad sizes n_points=%lld n_rings=%d",
                  (long long)n_points, n_rings);
  GLASS_CHECK_ARG(q4 >= 0 && q4 <= RS_MAX_Q4, "glass_ring_simplify_mark: q4=%d, the tolerance in quarter pixels, must be in 0..%d", q4,
                  RS_MAX_Q4);
  if (n_rings == 0) return GLASS_OK;
  GLASS_CHECK_ARG(out_off && status, "glass_ring_simplify_mark: null output");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int), st);
  if (e == hipSuccess && n_points == 0) e = hipMemsetAsync(out_off, 0, sizeof(int) * ((size_t)n_rings + 1), st);
  if (e != hipSuccess) {
    glass_set_error("glass_ring_simplify_mark: memset failed: %s", hipGetErrorString(e));
    return GLASS_EHIP;
  }
  if (n_points == 0) return GLASS_OK;
  GLASS_CHECK_ARG(xy && ring_off && workspace, "glass_ring_simplify_mark: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)xy & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
                  "glass_ring_simplify_mark: xy must be 8-byte and the workspace 16-byte aligned");
  GLASS_CHECK_ARG(workspace_bytes >= glass_ring_simplify_workspace_bytes(n_points, n_rings),
                  "glass_ring_simplify_mark: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)glass_ring_simplify_workspace_bytes(n_points, n_rings));
  int* counts = reinterpret_cast<int*>(workspace);
  unsigned char* flags = reinterpret_cast<unsigned char*>(workspace) + rs_align16((int64_t)n_rings * 4);
  hipLaunchKernelGGL(rs_mark_kernel, dim3(min(n_rings, RS_MAX_BLOCKS)), dim3(64), 0, st, reinterpret_cast<const int2*>(xy),
                     (long long)n_points, ring_off, n_rings, q4, flags, counts, status);
  GLASS_CHECK_LAUNCH("glass_ring_simplify_mark");
  hipLaunchKernelGGL(rs_offsets_kernel, dim3(1), dim3(RS_SCAN_THREADS), 0, st, counts, n_rings, out_off, status);
  GLASS_CHECK_LAUNCH("glass_ring_simplify_mark (offsets)");
  return GLASS_OK;
}

extern "C" int glass_ring_simplify_write(const int* xy, int64_t n_points, const int* ring_off, int n_rings, const void* workspace,
                                         int64_t workspace_bytes, const int* out_off, int* out_xy, int64_t n_out,
                                         glass_stream_t stream) {
  GLASS_CHECK_ARG(n_points >= 0 && n_points <= INT_MAX && n_rings >= 0 && n_out >= 0 && n_out <= n_points,
                  "glass_ring_simplify_write: bad sizes n_points=%lld n_rings=%d n_out=%lld", (long long)n_points, n_rings,
                  (long long)n_out);
  if (n_rings == 0 || n_points == 0 || n_out == 0) return GLASS_OK;
  GLASS_CHECK_ARG(xy && ring_off && workspace && out_off && out_xy, "glass_ring_simplify_write: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)xy & 7) == 0 && ((uintptr_t)out_xy & 7) == 0 && ((uintptr_t)workspace & 15) == 0,
                  "glass_ring_simplify_write: xy and out_xy must be 8-byte and the workspace 16-byte aligned");
  GLASS_CHECK_ARG(workspace_bytes >= glass_ring_simplify_workspace_bytes(n_points, n_rings),
                  "glass_ring_simplify_write: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)glass_ring_simplify_workspace_bytes(n_points, n_rings));
  const unsigned char* flags = reinterpret_cast<const unsigned char*>(workspace) + rs_align16((int64_t)n_rings * 4);
  hipLaunchKernelGGL(rs_write_kernel, dim3(min(n_rings, RS_MAX_BLOCKS)), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const int2*>(xy), (long long)n_points, ring_off, n_rings, flags, out_off,
                     reinterpret_cast<int2*>(out_xy), (long long)n_out);
  GLASS_CHECK_LAUNCH("glass_ring_simplify_write");
  return GLASS_OK;
}
