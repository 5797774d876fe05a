// glass_fuse_views (include/glass_hip_feature_fuse.h): the padded detections of V rotated and rescaled views of ONE image become
// one detection set in the image's frame, each survivor with the set of views that found it.  Per candidate: the ranking key
// (detection score, word score, or their product), the view's affine frame in float64, the bounds test on the centre; then a
// greedy pass in key order that compares boxes of DIFFERENT views only and, unlike merge_views_kernel, walks every candidate:
// a candidate that is not kept votes for the earliest kept box that overlaps it.  One workgroup of NMS_THREADS (16 wave64), the
// blocked form of merge_views_kernel / nms_select_kernel: sort keys in LDS, chunks of 64 sorted candidates, near pairs queued
// per wavefront for the polygon clipping.  The votes are final only after the walk, so the kept candidates' source slots and
// view masks stay in LDS and the output is written by one ordered compaction at the end.
#include <cmath>

#include "common.h"
#include "glass_hip_feature_fuse.h"
#include "proposal_common.h"
#include "rotated_iou.h"

constexpr int FV_VMAX = 64;      // a view is a bit of a 64-bit mask
constexpr int FV_TMAX = 64;
constexpr int FV_ROW = 8;        // floats of a candidate's workspace row: gx gy gw gh angle c2 s2 key
constexpr int FV_NONE = 0x7fffffff;

struct FuseParams {
  const float* boxes; const float* scores; const int* counts; const int* text_arg; const float* text_max;
  const double* affine; const float* bounds;
  int V, K, T, stop_index, rank_mode;
  float nms_thresh;
  int min_votes, max_out;
  float* out_boxes; float* out_scores; float* out_keys; int* out_src; int* out_votes; long long* out_views; int* out_count;
  float* rows;
};

// contract step 3: every value widened to float64, every product and sum rounded on its own, each result rounded to float32 once
__device__ __forceinline__ void fv_to_frame(const float* b, const double* m, float* g) {
#pragma clang fp contract(off)
  const double cx = b[0], cy = b[1];
  double a = (double)b[4] + m[7];
  a = a - 360.0 * floor((a + 180.0) / 360.0);
  g[0] = (float)(m[0] * cx + m[1] * cy + m[2]);
  g[1] = (float)(m[3] * cx + m[4] * cy + m[5]);
  g[2] = (float)((double)b[2] * m[6]);
  g[3] = (float)((double)b[3] * m[6]);
  g[4] = (float)a;
}

// LDS: dynamic = the sort keys, 8 B x npad (npad = V*K rounded up to a power of two, <= 8192: at most 64 KiB).  Static: kept
// boxes 1024 x 24 B = 24 KiB, their views 2 KiB, their source slots 4 KiB and view masks 8 KiB (the 12 KiB that
// merge_views_kernel does not have), the chunk's boxes 1.5 KiB, its masks 512 B, four int arrays 4 x 256 B, the pair queues
// 16 x 256 B = 4 KiB, the wavefront totals of the compaction and a few words: ~46 KiB.  Together at most ~110 KiB of the CU's
// 160 KiB; one workgroup per call, so occupancy is no concern.
__global__ __launch_bounds__(NMS_THREADS) void fuse_views_kernel(FuseParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];
  u64* order = reinterpret_cast<u64*>(dyn_smem);
  __shared__ RBox kept[NMS_KEEP_MAX];
  __shared__ unsigned short kview[NMS_KEEP_MAX];
  __shared__ int ksrc[NMS_KEEP_MAX];
  __shared__ u64 kmask[NMS_KEEP_MAX];
  __shared__ RBox chunk[64];
  __shared__ u64 cmask[64];
  __shared__ int cmin[64], cidx[64], cview[64], ckept[64];
  __shared__ unsigned short pair_queue[NMS_THREADS / 64][128];
  __shared__ int wave_total[NMS_THREADS / 64];
  __shared__ int s_nvalid, s_nkept, s_stop, s_cut, s_walked;

  const int total = p.V * p.K;
  int npad = 1;
  while (npad < total) npad <<= 1;

  // 1.-3. candidates, key, frame and bounds; sort keys (key descending, then view, then slot = flat index ascending)
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
          float key = sc;
          if (p.rank_mode != 0) {
            // the word score of the word post-processor (postprocess.hip): a float32 product in step order, up to and
            // including the first stop symbol
            float ws = 1.f;
            const long base = (long)idx * p.T;
            for (int t = 0; t < p.T; ++t) {
              ws *= p.text_max[base + t];
              if (p.text_arg[base + t] == p.stop_index) break;
            }
            key = p.rank_mode == 1 ? sc * ws : ws;
          }
          if (isfinite(key)) {
            double m[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = p.affine[8 * v + e];
            float g[5];
            fv_to_frame(b, m, g);
            if (isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(g[3]) && isfinite(g[4]) && g[2] > 0.f &&
                g[3] > 0.f && p.bounds[0] <= g[0] && g[0] <= p.bounds[2] && p.bounds[1] <= g[1] && g[1] <= p.bounds[3]) {
              const RBox r = make_rbox(g[0], g[1], g[2], g[3], g[4]);
              c = ((u64)float_key(key) << 32) | (u64)(0xffffffffu - (u32)idx);
              float4* row = reinterpret_cast<float4*>(p.rows + (long)idx * FV_ROW);
              row[0] = make_float4(g[0], g[1], g[2], g[3]);
              row[1] = make_float4(g[4], r.c2, r.s2, key);
            }
          }
        }
      }
    }
    order[idx] = c;
  }
  if (threadIdx.x == 0) { s_nkept = 0; s_stop = 0; s_cut = 0; }
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

  // 5. blocked greedy pass over chunks of 64 sorted candidates; pairs of one view count as far apart
  for (int c0 = 0; c0 < nvalid; c0 += 64) {
    const int csize = min(64, nvalid - c0);
    if (threadIdx.x < 64) {
      cmask[threadIdx.x] = 0;
      cmin[threadIdx.x] = FV_NONE;
      if ((int)threadIdx.x < csize) {
        // (a sorted composite holds an index below `total` by construction; clamped all the same before it addresses anything)
        const int idx = (int)min(0xffffffffu - (u32)(order[c0 + threadIdx.x] & 0xffffffffu), (u32)(total - 1));
        const float4* row = reinterpret_cast<const float4*>(p.rows + (long)idx * FV_ROW);
        const float4 a = row[0], b = row[1];
        RBox r;
        r.cx = a.x; r.cy = a.y; r.w = a.z; r.h = a.w; r.c2 = b.y; r.s2 = b.z;
        chunk[threadIdx.x] = r;
        cidx[threadIdx.x] = idx;
        cview[threadIdx.x] = idx / p.K;
      }
    }
    __syncthreads();
    const int nk = s_nkept;
    unsigned short* queue = pair_queue[threadIdx.x >> 6];
    // (a) candidates vs already kept boxes (i: kept box < 1024, j: candidate of the chunk): the earliest kept box that overlaps
    nms_for_pairs(csize * nk, queue, [&](int pr, int& i, int& j) { j = pr / nk; i = pr - j * nk; },
                  [&](int i, int j) { return (int)kview[i] == cview[j] || rbox_far_apart(kept[i], chunk[j]); },
                  [&](int i, int j) { if (rotated_iou(kept[i], chunk[j]) >= p.nms_thresh) atomicMin(&cmin[j], i); });
    // (b) intra-chunk pairs i < j
    nms_for_pairs(csize * csize, queue, [&](int pr, int& i, int& j) { i = pr / csize; j = pr - i * csize; },
                  [&](int i, int j) { return i >= j || cview[i] == cview[j] || rbox_far_apart(chunk[i], chunk[j]); },
                  [&](int i, int j) { if (rotated_iou(chunk[i], chunk[j]) >= p.nms_thresh) atomicOr(&cmask[i], 1ull << j); });
    __syncthreads();
    // (c) serial resolve inside the chunk, LDS only
    if (threadIdx.x == 0) {
      u64 sup = 0;
      int kcount = nk, walked = csize;
      for (int i = 0; i < csize; ++i) {
        ckept[i] = -1;
        if (cmin[i] != FV_NONE || ((sup >> i) & 1ull)) continue;
        kept[kcount] = chunk[i];
        kview[kcount] = (unsigned short)cview[i];
        ksrc[kcount] = cidx[i];
        kmask[kcount] = 1ull << cview[i];
        ckept[i] = kcount;
        ++kcount;
        sup |= cmask[i];
        if (kcount >= NMS_KEEP_MAX) {        // the 1024th kept place is taken: what follows is neither kept nor a supporter
          s_stop = 1;
          s_cut = (c0 + i + 1 < nvalid) ? 1 : 0;
          walked = i + 1;
          break;
        }
      }
      s_nkept = kcount;
      s_walked = walked;
    }
    __syncthreads();
    // (d) 6. a candidate that was not kept supports the earliest kept box that overlaps it: one of an earlier chunk if there is
    // one (they all precede the chunk's own), otherwise its first kept predecessor inside the chunk
    if ((int)threadIdx.x < s_walked && ckept[threadIdx.x] < 0) {
      const int j = threadIdx.x;
      int target = cmin[j] != FV_NONE ? cmin[j] : -1;
      if (target < 0) {
        for (int i = 0; i < j; ++i)
          if (ckept[i] >= 0 && ((cmask[i] >> j) & 1ull)) { target = ckept[i]; break; }
      }
      if (target >= 0 && target < NMS_KEEP_MAX) atomicOr(&kmask[target], 1ull << cview[j]);
    }
    __syncthreads();
    if (s_stop) break;
  }

  // 7. ordered compaction of the kept candidates with enough votes (kept index t on thread t: NMS_KEEP_MAX == NMS_THREADS)
  const int nkept = s_nkept;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  u64 views = 0;
  int votes = 0;
  if (t < nkept) { views = kmask[t]; votes = __popcll(views); }
  const bool pass = t < nkept && votes >= p.min_votes;
  const u64 ball = __ballot(pass);
  if (lane == 0) wave_total[wave] = __popcll(ball);
  __syncthreads();
  int before = 0, n = 0;
  for (int w = 0; w < NMS_THREADS / 64; ++w) {
    const int c = wave_total[w];
    if (w < wave) before += c;
    n += c;
  }
  const int o = before + __popcll(ball & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
  if (pass && o < p.max_out) {
    const int idx = ksrc[t];
    const float4* row = reinterpret_cast<const float4*>(p.rows + (long)idx * FV_ROW);
    const float4 a = row[0], b = row[1];
    p.out_boxes[o * 5 + 0] = a.x; p.out_boxes[o * 5 + 1] = a.y; p.out_boxes[o * 5 + 2] = a.z; p.out_boxes[o * 5 + 3] = a.w;
    p.out_boxes[o * 5 + 4] = b.x;
    p.out_scores[o] = p.scores[idx];
    p.out_keys[o] = b.w;
    p.out_src[o] = idx;
    p.out_votes[o] = votes;
    p.out_views[o] = (long long)views;
  }
  if (t == 0) {
    p.out_count[0] = min(n, p.max_out);
    p.out_count[1] = (s_cut || n > p.max_out) ? 1 : 0;
    p.out_count[2] = nkept;
  }
}

static_assert(NMS_KEEP_MAX == NMS_THREADS, "the final compaction gives kept candidate t to thread t");

static bool fv_check_shape(int V, int K) {
  return V >= 0 && V <= FV_VMAX && K >= 1 && K <= NMS_KEEP_MAX && (long)V * K <= NMS_SMAX;
}

extern "C" int64_t glass_fuse_views_workspace_bytes(int V, int K) {
  if (!fv_check_shape(V, K)) {
    glass_set_error("glass_fuse_views_workspace_bytes: V=%d K=%d (0 <= V <= %d, 1 <= K <= %d, V*K <= %d)", V, K, FV_VMAX,
                    NMS_KEEP_MAX, NMS_SMAX);
    return GLASS_EINVAL;
  }
  return (int64_t)sizeof(float) * FV_ROW * (V * K > 0 ? V * K : 1);
}

extern "C" int glass_fuse_views(const float* boxes, const float* scores, const int* counts, const int* text_arg,
                                const float* text_max, int T, int stop_index, int rank_mode, const double* view_affine,
                                const float* bounds, int V, int K, float nms_thresh, int min_votes, int max_out, float* out_boxes,
                                float* out_scores, float* out_keys, int* out_src, int* out_votes, int64_t* out_views,
                                int* out_count, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(fv_check_shape(V, K), "glass_fuse_views: V=%d K=%d (0 <= V <= %d, 1 <= K <= %d, V*K <= %d)", V, K, FV_VMAX,
                  NMS_KEEP_MAX, NMS_SMAX);
  GLASS_CHECK_ARG(rank_mode >= 0 && rank_mode <= 2, "glass_fuse_views: rank_mode=%d (0 detection, 1 product, 2 word)", rank_mode);
  GLASS_CHECK_ARG(stop_index >= 0, "glass_fuse_views: stop_index=%d", stop_index);
  GLASS_CHECK_ARG(rank_mode == 0 || (T >= 1 && T <= FV_TMAX), "glass_fuse_views: T=%d (1..%d)", T, FV_TMAX);
  GLASS_CHECK_ARG(min_votes >= 1 && min_votes <= FV_VMAX, "glass_fuse_views: min_votes=%d (1..%d)", min_votes, FV_VMAX);
  GLASS_CHECK_ARG(max_out >= 1 && max_out <= NMS_KEEP_MAX, "glass_fuse_views: max_out=%d (1..%d)", max_out, NMS_KEEP_MAX);
  GLASS_CHECK_ARG(std::isfinite(nms_thresh), "glass_fuse_views: nms_thresh is not finite");
  GLASS_CHECK_ARG(out_boxes && out_scores && out_keys && out_src && out_votes && out_views && out_count,
                  "glass_fuse_views: null output pointer");
  if (V == 0) {
    hipError_t e = hipMemsetAsync(out_count, 0, sizeof(int) * 3, (hipStream_t)stream);
    if (e != hipSuccess) { glass_set_error("glass_fuse_views: memset: %s", hipGetErrorString(e)); return GLASS_EHIP; }
    return GLASS_OK;
  }
  GLASS_CHECK_ARG(boxes && scores && counts && view_affine && bounds, "glass_fuse_views: null input pointer");
  GLASS_CHECK_ARG(rank_mode == 0 || (text_arg && text_max), "glass_fuse_views: null text pointer with rank_mode=%d", rank_mode);
  const int64_t need = glass_fuse_views_workspace_bytes(V, K);
  GLASS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                  "glass_fuse_views: workspace of %lld bytes (needs %lld, 16-byte aligned)", (long long)workspace_bytes,
                  (long long)need);
  int npad = 1;
  while (npad < V * K) npad <<= 1;
  const size_t smem = sizeof(u64) * npad;
  FuseParams p;
  p.boxes = boxes; p.scores = scores; p.counts = counts; p.text_arg = text_arg; p.text_max = text_max;
  p.affine = view_affine; p.bounds = bounds;
  p.V = V; p.K = K; p.T = rank_mode == 0 ? 0 : T; p.stop_index = stop_index; p.rank_mode = rank_mode;
  p.nms_thresh = nms_thresh; p.min_votes = min_votes; p.max_out = max_out;
  p.out_boxes = out_boxes; p.out_scores = out_scores; p.out_keys = out_keys; p.out_src = out_src; p.out_votes = out_votes;
  p.out_views = reinterpret_cast<long long*>(out_views); p.out_count = out_count;
  p.rows = static_cast<float*>(workspace);
  // on every call, not once per process: the attribute belongs to the device that is current, and the call is cheap.  64 KiB:
  // the sort keys at V*K = 8192 (the static ~46 KiB come on top)
  const int attr_rc = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(fuse_views_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  if (attr_rc != 0) {
    glass_set_error("glass_fuse_views: cannot raise the dynamic LDS limit (hip error %d)", attr_rc);
    return GLASS_EHIP;
  }
  hipLaunchKernelGGL(fuse_views_kernel, dim3(1), dim3(NMS_THREADS), smem, (hipStream_t)stream, p);
  GLASS_CHECK_LAUNCH("glass_fuse_views");
  return GLASS_OK;
}
