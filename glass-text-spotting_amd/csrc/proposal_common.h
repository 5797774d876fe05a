// Shared device helpers of the proposal kernels (proposals.hip, rpn.hip, view_merge.hip).
#pragma once
#include "common.h"
#include "rotated_iou.h"

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr float SCALE_CLAMP = 4.135166556742356f;  // log(1000/16), d2 Box2BoxTransformRotated

__device__ __forceinline__ u32 float_key(float f) {
  // order-preserving map float -> uint (larger float => larger key); -0.0 and +0.0 compare equal in
  // torch.sort, so both map to the key of +0.0 (a stable sort then orders them by index)
  u32 u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(u32 k) {
  u32 u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// descending bitonic sort of `npad` (power of two) u64 in LDS by all threads of the block
__device__ inline void bitonic_sort_desc(u64* a, int npad) {
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const u64 x = a[i], y = a[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) { a[i] = y; a[ixj] = x; }
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ float floor_mod(float a, float b) {  // torch.remainder semantics
  float m = fmodf(a, b);
  if (m != 0.f && ((b < 0.f) != (m < 0.f))) m += b;
  return m;
}

// ------------------------------------------------------------------ pieces of the blocked greedy NMS (proposals.hip nms_select_kernel,
// view_merge.hip merge_views_kernel): one workgroup of NMS_THREADS, chunks of 64 sorted candidates
constexpr int NMS_SMAX = 8192;
constexpr int NMS_KEEP_MAX = 1024;
constexpr int NMS_THREADS = 1024;

// the early exit of rotated_iou (rotated_iou.h: circumscribed circles disjoint -> IoU exactly 0), as a predicate of its own
__device__ __forceinline__ bool rbox_far_apart(const RBox& a, const RBox& b) {
#pragma clang fp contract(off)
  const float dx = a.cx - b.cx, dy = a.cy - b.cy;
  const float rr = 0.5f * (sqrtf(a.w * a.w + a.h * a.h) + sqrtf(b.w * b.w + b.h * b.h));
  return dx * dx + dy * dy > rr * rr * 1.001f + 1e-2f;
}

// `total` box pairs, pair pr -> (i, j) by `decode`; the pairs that are not far apart - the ones that run the polygon clipping,
// whose point lists live in scratch - are collected per wavefront (ballot compaction, 128 entries each) and evaluated 64 at a
// time with every lane busy, instead of by whichever lanes of a round happen to hold one (postprocess.hip: pp_for_pairs).
template <class Decode, class Far, class Heavy>
__device__ __forceinline__ void nms_for_pairs(int total, unsigned short* queue, Decode decode, Far far, Heavy heavy) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int qn = 0;                                                       // (wavefront-uniform)
  for (int base = threadIdx.x & ~63; base < total; base += NMS_THREADS) {
    const int pr = base + lane;
    int i = 0, j = 0;
    bool near = false;
    if (pr < total) {
      decode(pr, i, j);
      near = !far(i, j);
    }
    const unsigned long long m = __ballot(near);
    if (near) queue[qn + __popcll(m & below)] = (unsigned short)((i << 6) | j);
    qn += __popcll(m);
    if (qn >= 64) {
      qn -= 64;
      const int e = queue[qn + lane];
      heavy(e >> 6, e & 63);
    }
  }
  if (lane < qn) {
    const int e = queue[lane];
    heavy(e >> 6, e & 63);
  }
}
