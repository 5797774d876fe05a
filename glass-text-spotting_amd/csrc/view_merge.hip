// glass_merge_views (include/glass_hip_ext_views.h): the padded detections of V views of ONE image - overlapping tiles, plus
// a low-resolution view of the whole image - become one detection set in the image's frame.  Per candidate: the view's
// frame transform, its keep rectangle (a word cut by an interior tile edge is dropped) and its size band; then a greedy
// suppression in score order that compares boxes of DIFFERENT views only (the opposite of glass_rotated_nms_select, which
// compares boxes of one category only).  One workgroup of NMS_THREADS (16 wave64), the blocked form of nms_select_kernel:
// sort keys in LDS, chunks of 64 sorted candidates, near pairs queued per wavefront for the polygon clipping.
#include <cmath>

#include "common.h"
#include "glass_hip_ext_views.h"
#include "proposal_common.h"
#include "rotated_iou.h"

constexpr int MV_VMAX = 256;
constexpr int MV_ROW = 8;      // floats of a candidate's workspace row: gx gy gw gh angle c2 s2 -

struct MergeParams {
  const float* boxes; const float* scores; const int* counts; const float* xform; const float* keep; const float* band;
  int V, K;
  float nms_thresh;
  int max_out;
  float* out_boxes; float* out_scores; int* out_src; int* out_count;
  float* rows;
};

// the global box of contract step 2: every product and sum rounded separately, so that a float32 replay on the host gives
// the same bits
__device__ __forceinline__ void mv_to_frame(const float* b, float ox, float oy, float inv, float* g) {
#pragma clang fp contract(off)
  g[0] = b[0] * inv + ox;
  g[1] = b[1] * inv + oy;
  g[2] = b[2] * inv;
  g[3] = b[3] * inv;
  g[4] = b[4];
}

// LDS: dynamic = the sort keys, 8 B x npad (npad = V*K rounded up to a power of two, <= 8192: at most 64 KiB).  Static:
// kept boxes 1024 x 24 B = 24 KiB, their views 2 KiB, the chunk's boxes 1.5 KiB, masks / flags / slots / views / output slots
// of the chunk 5 x 256 B + 512 B, its output rows 1.5 KiB, the pair queues 16 x 256 B = 4 KiB, a few words: ~35 KiB.
// Together at most ~99 KiB of the CU's 160 KiB; one workgroup per call, so occupancy is no concern.
__global__ __launch_bounds__(NMS_THREADS) void merge_views_kernel(MergeParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  u64* order = reinterpret_cast<u64*>(dyn_smem);
  __shared__ RBox kept[NMS_KEEP_MAX];
  __shared__ unsigned short kview[NMS_KEEP_MAX];
  __shared__ RBox chunk[64];
  __shared__ u64 cmask[64];
  __shared__ int csup[64], cidx[64], cview[64], ckept[64];
  __shared__ float cbox[64][5], cscore[64];
  __shared__ unsigned short pair_queue[NMS_THREADS / 64][128];
  __shared__ int s_nvalid, s_nkept, s_stop, s_more;

  const int total = p.V * p.K;
  int npad = 1;
  while (npad < total) npad <<= 1;

  // 1.-3. candidates, frame, border and size band; sort keys (score descending, then view, then slot = flat index ascending)
  for (int idx = threadIdx.x; idx < npad; idx += blockDim.x) {
    u64 c = 0;
    if (idx < total) {
      const int v = idx / p.K, s = idx - v * p.K;
      const int cnt = min(max(p.counts[v], 0), p.K);
      if (s < cnt) {
        const float sc = p.scores[idx];
        float b[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) b[e] = p.boxes[(long)idx * 5 + e];
        if (isfinite(sc) && isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]) && isfinite(b[4])) {
          float g[5];
          mv_to_frame(b, p.xform[3 * v], p.xform[3 * v + 1], p.xform[3 * v + 2], g);
          if (g[2] > 0.f && g[3] > 0.f) {
            const RBox r = make_rbox(g[0], g[1], g[2], g[3], g[4]);
            Pt pts[4];
            rbox_vertices(r.cx, r.cy, r, pts);
            const float xmin = fminf(fminf(pts[0].x, pts[1].x), fminf(pts[2].x, pts[3].x));
            const float xmax = fmaxf(fmaxf(pts[0].x, pts[1].x), fmaxf(pts[2].x, pts[3].x));
            const float ymin = fminf(fminf(pts[0].y, pts[1].y), fminf(pts[2].y, pts[3].y));
            const float ymax = fmaxf(fmaxf(pts[0].y, pts[1].y), fmaxf(pts[2].y, pts[3].y));
            const float size = fmaxf(xmax - xmin, ymax - ymin);
            const float* kr = p.keep + 4 * v;
            if (kr[0] <= xmin && xmax <= kr[2] && kr[1] <= ymin && ymax <= kr[3] && p.band[2 * v] < size &&
                size <= p.band[2 * v + 1]) {
              c = ((u64)float_key(sc) << 32) | (u64)(0xffffffffu - (u32)idx);
              float4* row = reinterpret_cast<float4*>(p.rows + (long)idx * MV_ROW);
              row[0] = make_float4(g[0], g[1], g[2], g[3]);
              row[1] = make_float4(g[4], r.c2, r.s2, 0.f);
            }
          }
        }
      }
    }
    order[idx] = c;
  }
  if (threadIdx.x == 0) { s_nkept = 0; s_stop = 0; s_more = 0; }
  __syncthreads();                       // (also orders the workspace rows before their reads by other threads below)
  // 4. order
  bitonic_sort_desc(order, npad);
  // valid composites are never 0 (their low word is 0xffffffff - idx with idx < 8192), so the first zero ends them
  if (threadIdx.x == 0) {
    int lo = 0, hi = npad;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (order[mid] != 0) lo = mid + 1; else hi = mid; }
    s_nvalid = lo;
  }
  __syncthreads();
  const int nvalid = s_nvalid;

  // 5. blocked greedy suppression over chunks of 64 sorted candidates; pairs of one view count as far apart
  for (int c0 = 0; c0 < nvalid; c0 += 64) {
    const int csize = min(64, nvalid - c0);
    if (threadIdx.x < 64) {
      cmask[threadIdx.x] = 0;
      csup[threadIdx.x] = 0;
      if ((int)threadIdx.x < csize) {
        const int idx = (int)(0xffffffffu - (u32)(order[c0 + threadIdx.x] & 0xffffffffu));
        const float4* row = reinterpret_cast<const float4*>(p.rows + (long)idx * MV_ROW);
        const float4 a = row[0], b = row[1];
        RBox r;
        r.cx = a.x; r.cy = a.y; r.w = a.z; r.h = a.w; r.c2 = b.y; r.s2 = b.z;
        chunk[threadIdx.x] = r;
        cidx[threadIdx.x] = idx;
        cview[threadIdx.x] = idx / p.K;
        cbox[threadIdx.x][0] = a.x; cbox[threadIdx.x][1] = a.y; cbox[threadIdx.x][2] = a.z; cbox[threadIdx.x][3] = a.w;
        cbox[threadIdx.x][4] = b.x;
        cscore[threadIdx.x] = p.scores[idx];
      }
    }
    __syncthreads();
    const int nk = s_nkept;
    unsigned short* queue = pair_queue[threadIdx.x >> 6];
    // (a) candidates vs already kept boxes (i: kept box < 1024, j: candidate of the chunk)
    nms_for_pairs(csize * nk, queue, [&](int pr, int& i, int& j) { j = pr / nk; i = pr - j * nk; },
                  [&](int i, int j) { return (int)kview[i] == cview[j] || rbox_far_apart(kept[i], chunk[j]); },
                  [&](int i, int j) { if (rotated_iou(kept[i], chunk[j]) >= p.nms_thresh) csup[j] = 1; });
    // (b) intra-chunk pairs i < j
    nms_for_pairs(csize * csize, queue, [&](int pr, int& i, int& j) { i = pr / csize; j = pr - i * csize; },
                  [&](int i, int j) { return i >= j || cview[i] == cview[j] || rbox_far_apart(chunk[i], chunk[j]); },
                  [&](int i, int j) { if (rotated_iou(chunk[i], chunk[j]) >= p.nms_thresh) atomicOr(&cmask[i], 1ull << j); });
    __syncthreads();
    // (c) serial resolve inside the chunk, LDS only
    if (threadIdx.x == 0) {
      u64 sup = 0;
      int kcount = nk;
      for (int i = 0; i < csize; ++i) {
        ckept[i] = -1;
        if (csup[i] || ((sup >> i) & 1ull)) continue;
        kept[kcount] = chunk[i];
        kview[kcount] = (unsigned short)cview[i];
        ckept[i] = kcount;
        ++kcount;
        sup |= cmask[i];
        if (kcount >= p.max_out) {           // the max_out-th candidate is kept: anything after it in the order is cut off
          s_stop = 1;
          s_more = (c0 + i + 1 < nvalid) ? 1 : 0;
          for (int j = i + 1; j < csize; ++j) ckept[j] = -1;
          break;
        }
      }
      s_nkept = kcount;
    }
    __syncthreads();
    // 6. output rows of the chunk's survivors
    if ((int)threadIdx.x < csize && ckept[threadIdx.x] >= 0) {
      const int o = ckept[threadIdx.x];
#pragma unroll
      for (int e = 0; e < 5; ++e) p.out_boxes[o * 5 + e] = cbox[threadIdx.x][e];
      p.out_scores[o] = cscore[threadIdx.x];
      p.out_src[o] = cidx[threadIdx.x];
    }
    if (s_stop) break;
  }
  if (threadIdx.x == 0) { p.out_count[0] = s_nkept; p.out_count[1] = s_more; }
}

static bool mv_check_shape(int V, int K) {
  return V >= 0 && V <= MV_VMAX && K >= 1 && K <= NMS_KEEP_MAX && (long)V * K <= NMS_SMAX;
}

extern "C" int64_t glass_merge_views_workspace_bytes(int V, int K) {
  if (!mv_check_shape(V, K)) {
    glass_set_error("glass_merge_views_workspace_bytes: V=%d K=%d (0 <= V <= %d, 1 <= K <= %d, V*K <= %d)", V, K, MV_VMAX,
                    NMS_KEEP_MAX, NMS_SMAX);
    return GLASS_EINVAL;
  }
  return (int64_t)sizeof(float) * MV_ROW * (V * K > 0 ? V * K : 1);
}

extern "C" int glass_merge_views(const float* boxes, const float* scores, const int* counts, const float* view_xform,
                                 const float* keep_rect, const float* size_range, int V, int K, float nms_thresh, int max_out,
                                 float* out_boxes, float* out_scores, int* out_src, int* out_count, void* workspace,
                                 int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(mv_check_shape(V, K), "glass_merge_views: V=%d K=%d (0 <= V <= %d, 1 <= K <= %d, V*K <= %d)", V, K, MV_VMAX,
                  NMS_KEEP_MAX, NMS_SMAX);
  GLASS_CHECK_ARG(max_out >= 1 && max_out <= NMS_KEEP_MAX, "glass_merge_views: max_out=%d (1..%d)", max_out, NMS_KEEP_MAX);
  GLASS_CHECK_ARG(std::isfinite(nms_thresh), "glass_merge_views: nms_thresh is not finite");
  GLASS_CHECK_ARG(out_boxes && out_scores && out_src && out_count, "glass_merge_views: null output pointer");
  if (V == 0) {
    hipError_t e = hipMemsetAsync(out_count, 0, sizeof(int) * 2, (hipStream_t)stream);
    if (e != hipSuccess) { glass_set_error("glass_merge_views: memset: %s", hipGetErrorString(e)); return GLASS_EHIP; }
    return GLASS_OK;
  }
  GLASS_CHECK_ARG(boxes && scores && counts && view_xform && keep_rect && size_range, "glass_merge_views: null input pointer");
  const int64_t need = glass_merge_views_workspace_bytes(V, K);
  GLASS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                  "glass_merge_views: workspace of %lld bytes (needs %lld, 16-byte aligned)", (long long)workspace_bytes,
                  (long long)need);
  int npad = 1;
  while (npad < V * K) npad <<= 1;
  const size_t smem = sizeof(u64) * npad;
  MergeParams p;
  p.boxes = boxes; p.scores = scores; p.counts = counts; p.xform = view_xform; p.keep = keep_rect; p.band = size_range;
  p.V = V; p.K = K; p.nms_thresh = nms_thresh; p.max_out = max_out;
  p.out_boxes = out_boxes; p.out_scores = out_scores; p.out_src = out_src; p.out_count = out_count;
  p.rows = static_cast<float*>(workspace);
  static const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(merge_views_kernel),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);       // 64 KiB of sort keys at V*K = 8192 (the static ~35 KiB come on top)
  if (attr_rc != 0) {
    glass_set_error("glass_merge_views: cannot raise the dynamic LDS limit (hip error %d)", attr_rc);
    return GLASS_EHIP;
  }
  hipLaunchKernelGGL(merge_views_kernel, dim3(1), dim3(NMS_THREADS), smem, (hipStream_t)stream, p);
  GLASS_CHECK_LAUNCH("glass_merge_views");
  return GLASS_OK;
}
