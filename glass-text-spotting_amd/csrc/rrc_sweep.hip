// Threshold sweep of the RRC protocol (glass_rrc_sweep): the tallies of csrc/rrc_score.hip's decisions for K pairs of
// (text, detection) confidence thresholds from one set of pair areas.
//
// Under the protocol a threshold only removes detections: the don't-care mark of a detection depends on that detection and
// the ground truth alone, the intersection areas are per pair, and the matching is "GT in order, each care GT takes the
// lowest care, unmatched, present detection with IoU > 0.5".  So the candidate relation of an image, IoU > 0.5 with exactly
// the fp64 operations of rrc_match_kernel, is one G x D bit matrix for every combination, and what is left per
// (image, combination) is a small integer problem on 64-bit words.
//
// Two launches.  rrc_sweep_bits_kernel, one workgroup per image: the matrix as ceil(D / 64) words per GT row (a wave per
// word: lane = detection, ballot) and, per care set, the words of the detections without the don't-care mark, into the
// workspace.  rrc_sweep_kernel, one workgroup per (slice of 256 combinations, group of images), one lane per combination:
// the lane forms its present mask with D compares, then runs the greedy pass of each care set as
// row[g] & care & present & ~taken, first set bit, serially over G and over the words in order.  The rows of an image are
// copied to LDS when they fit RRC_SWEEP_LDS_WORDS and read from the workspace otherwise; all lanes read the same row word
// at the same time (a broadcast), only their masks differ.  A lane keeps its masks in registers up to 8 words (D <= 512)
// and in a workspace slot of its own above that.  A lane adds the images of its group in registers and then adds its six
// totals into counts[k] with integer atomics: the order of the adds is free and the result exact, so two runs are
// identical.  No waiting on another workgroup, every loop bounded by a size read once.
//
// Workspace slots without a prefix sum: image i (GT polygons g0 .., detections d0 .., pairs from p0) has its rows at word
// p0 / 64 + 2 * (g0 - gt_off[0]) and its care words at (d0 - det_off[0]) / 64 + i.  Consecutive slots do not overlap:
// floor((p0 + G D) / 64) - floor(p0 / 64) + 2 G >= floor(G D / 64) + 2 G >= G * ceil(D / 64) for G >= 1, and
// floor((d + D) / 64) - floor(d / 64) + 1 > D / 64, an integer, so >= ceil(D / 64).
#include "common.h"

namespace {

constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_REG_WORDS = 8;                        // masks of up to this many words stay in registers
constexpr int SWEEP_MAX_BLOCKS = 4096;                    // workgroups of the sweep (images are grouped to stay near it)
constexpr int SWEEP_MAX_BLOCKS_SPILL = 256;               // ... when every lane needs a mask slot in the workspace
constexpr int SWEEP_NO_WORD = -2;                         // det_word below 0 matches nothing (gt_accept pads with -1)

typedef unsigned long long u64;

struct SweepImage {
  int g0, d0, G, D, W;
  long long base, row_off, care_off;
};

// the image's ranges, or false when they leave the arrays (uniform over the workgroup; the host never builds such an image)
__device__ __forceinline__ bool sweep_image(const long long* __restrict__ pair_off, const int* __restrict__ gt_off,
                                            const int* __restrict__ det_off, int img, int n_poly, int n_gt, int n_det,
                                            long long n_pairs, int max_dets, SweepImage& s) {
  const int gbase = gt_off[0], dbase = det_off[0];
  s.g0 = gt_off[img];
  s.d0 = det_off[img];
  s.G = gt_off[img + 1] - s.g0;
  s.D = det_off[img + 1] - s.d0;
  s.base = pair_off[img];
  if (s.G < 0 || s.D < 0 || s.D > max_dets || s.g0 < 0 || s.d0 < 0 || (long)s.g0 + s.G > n_poly || (long)s.d0 + s.D > n_poly ||
      s.g0 - gbase < 0 || s.g0 - gbase + s.G > n_gt || s.d0 - dbase < 0 || s.d0 - dbase + s.D > n_det || s.base < 0 ||
      s.base + (long long)s.G * s.D > n_pairs)
    return false;
  s.W = (s.D + 63) >> 6;
  s.row_off = (s.base >> 6) + 2ll * (s.g0 - gbase);
  s.care_off = ((s.d0 - dbase) >> 6) + img;
  s.g0 -= gbase;                                                        // from here on: indices into the chunk's arrays
  s.d0 -= dbase;
  return true;
}

__global__ __launch_bounds__(SWEEP_THREADS) void rrc_sweep_bits_kernel(
    const double* __restrict__ area, int n_poly, const double* __restrict__ inter, long long n_pairs,
    const long long* __restrict__ pair_off, const int* __restrict__ gt_off, const int* __restrict__ det_off, int I, int n_gt,
    int n_det, int max_dets, const unsigned char* __restrict__ det_dc_e2e, const unsigned char* __restrict__ det_dc_det,
    u64* __restrict__ rows, u64* __restrict__ care_e2e, u64* __restrict__ care_det) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int gbase = gt_off[0], dbase = det_off[0];
  for (int img = blockIdx.x; img < I; img += gridDim.x) {
    SweepImage s;
    if (!sweep_image(pair_off, gt_off, det_off, img, n_poly, n_gt, n_det, n_pairs, max_dets, s)) continue;
    const long long words = (long long)s.G * s.W;
    for (long long idx = wid; idx < words; idx += SWEEP_THREADS / 64) {    // wave-uniform
      const int g = (int)(idx / s.W), w = (int)(idx - (long long)g * s.W);
      const int d = w * 64 + lane;
      bool ok = false;
      if (d < s.D) {                                                    // the operations of rrc_match_kernel, in its order
        const double ag = area[gbase + s.g0 + g];
        const double in = inter[s.base + (long long)g * s.D + d];
        const double un = ag + area[dbase + s.d0 + d] - in;
        ok = (un == 0.0 ? 0.0 : in / un) > 0.5;
      }
      const u64 b = __ballot(ok);
      if (lane == 0) rows[s.row_off + idx] = b;
    }
    for (int w = wid; w < s.W; w += SWEEP_THREADS / 64) {
      const int d = w * 64 + lane;
      const u64 be = __ballot(d < s.D && !det_dc_e2e[s.d0 + d]);
      const u64 bd = __ballot(d < s.D && !det_dc_det[s.d0 + d]);
      if (lane == 0) {
        care_e2e[s.care_off + w] = be;
        care_det[s.care_off + w] = bd;
      }
    }
  }
}

// bit b of word w: detection w * 64 + b passes both thresholds (a score equal to its threshold stays)
__device__ __forceinline__ u64 present_word(const double* __restrict__ score_text, const double* __restrict__ score_det, int d_begin,
                                            int n, double text_th, double det_th) {
  u64 word = 0;
  for (int b = 0; b < n; ++b) {
    const bool p = !(score_text[d_begin + b] < text_th) && !(score_det[d_begin + b] < det_th);
    word |= (u64)p << b;
  }
  return word;
}

__device__ __forceinline__ bool accepts(const int* __restrict__ gt_accept, int g, int word) {
  const int4 a = reinterpret_cast<const int4*>(gt_accept)[g];
  return word >= 0 && (word == a.x || word == a.y || word == a.z || word == a.w);
}

// One image for one lane, masks in registers (NW words, W <= NW of them in use).  `rows` is LDS or the workspace.
template <int NW>
__device__ __forceinline__ void sweep_lane(const u64* rows, const SweepImage& s, const u64* __restrict__ care_e2e,
                                           const u64* __restrict__ care_det, const unsigned char* __restrict__ gt_dc_e2e,
                                           const unsigned char* __restrict__ gt_dc_det, const double* __restrict__ score_text,
                                           const double* __restrict__ score_det, const int* __restrict__ gt_accept,
                                           const int* __restrict__ det_word, double text_th, double det_th, long long* acc) {
  u64 present[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w)
    present[w] = w < s.W ? present_word(score_text, score_det, s.d0 + w * 64, min(64, s.D - w * 64), text_th, det_th) : 0;
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    const u64* care = (set ? care_det : care_e2e) + s.care_off;
    const unsigned char* gt_dc = (set ? gt_dc_det : gt_dc_e2e) + s.g0;
    u64 avail[NW];
    int det_care = 0, matched = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      avail[w] = w < s.W ? present[w] & care[w] : 0;
      det_care += __popcll(avail[w]);
    }
    for (int g = 0; g < s.G; ++g) {
      if (gt_dc[g]) continue;                                           // uniform over the workgroup
      int d = -1;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w < s.W && d < 0) {
          const u64 m = rows[(long long)g * s.W + w] & avail[w];
          if (m) {
            d = w * 64 + __ffsll((long long)m) - 1;
            avail[w] &= ~(m & (0 - m));
          }
        }
      }
      if (d >= 0) matched += set ? 1 : (accepts(gt_accept, s.g0 + g, det_word[s.d0 + d]) ? 1 : 0);
    }
    acc[set * 3 + 0] += matched;
    acc[set * 3 + 2] += det_care;
  }
}

// The same with the masks in the lane's workspace slot: word w of the present mask at slot[w * SWEEP_THREADS], of the
// available mask at slot[(max_words + w) * SWEEP_THREADS] (neighbouring lanes are neighbours in memory).
__device__ __forceinline__ void sweep_lane_spill(const u64* rows, const SweepImage& s, const u64* __restrict__ care_e2e,
                                                 const u64* __restrict__ care_det, const unsigned char* __restrict__ gt_dc_e2e,
                                                 const unsigned char* __restrict__ gt_dc_det, const double* __restrict__ score_text,
                                                 const double* __restrict__ score_det, const int* __restrict__ gt_accept,
                                                 const int* __restrict__ det_word, double text_th, double det_th, long long* acc,
                                                 u64* slot, int max_words) {
  u64* present = slot;
  u64* avail = slot + (long long)max_words * SWEEP_THREADS;
  for (int w = 0; w < s.W; ++w)
    present[(long long)w * SWEEP_THREADS] = present_word(score_text, score_det, s.d0 + w * 64, min(64, s.D - w * 64), text_th, det_th);
  for (int set = 0; set < 2; ++set) {
    const u64* care = (set ? care_det : care_e2e) + s.care_off;
    const unsigned char* gt_dc = (set ? gt_dc_det : gt_dc_e2e) + s.g0;
    int det_care = 0, matched = 0;
    for (int w = 0; w < s.W; ++w) {
      const u64 a = present[(long long)w * SWEEP_THREADS] & care[w];
      avail[(long long)w * SWEEP_THREADS] = a;
      det_care += __popcll(a);
    }
    for (int g = 0; g < s.G; ++g) {
      if (gt_dc[g]) continue;
      int d = -1;
      for (int w = 0; w < s.W && d < 0; ++w) {
        const u64 a = avail[(long long)w * SWEEP_THREADS];
        const u64 m = rows[(long long)g * s.W + w] & a;
        if (m) {
          d = w * 64 + __ffsll((long long)m) - 1;
          avail[(long long)w * SWEEP_THREADS] = a & ~(m & (0 - m));
        }
      }
      if (d >= 0) matched += set ? 1 : (accepts(gt_accept, s.g0 + g, det_word[s.d0 + d]) ? 1 : 0);
    }
    acc[set * 3 + 0] += matched;
    acc[set * 3 + 2] += det_care;
  }
}

#define SWEEP_LANE(NW, ROWS) \
  sweep_lane<NW>(ROWS, s, care_e2e, care_det, gt_dc_e2e, gt_dc_det, score_text, score_det, gt_accept, det_word, tt, dt, acc)

__global__ __launch_bounds__(SWEEP_THREADS) void rrc_sweep_kernel(
    int n_poly, long long n_pairs, const long long* __restrict__ pair_off, const int* __restrict__ gt_off,
    const int* __restrict__ det_off, int I, const unsigned char* __restrict__ gt_dc_e2e, const unsigned char* __restrict__ gt_dc_det,
    int n_gt, int n_det, int max_dets, const double* __restrict__ score_text, const double* __restrict__ score_det,
    const int* __restrict__ gt_accept, const int* __restrict__ det_word, const double* __restrict__ text_th,
    const double* __restrict__ det_th, int K, const u64* __restrict__ rows, const u64* __restrict__ care_e2e,
    const u64* __restrict__ care_det, u64* spill, int max_words, u64* counts) {
  __shared__ u64 lds_rows[GLASS_RRC_SWEEP_LDS_WORDS];
  const int tid = threadIdx.x;
  const int n_slices = (K + SWEEP_THREADS - 1) / SWEEP_THREADS;
  u64* slot = spill ? spill + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * max_words * SWEEP_THREADS + tid : nullptr;
  for (int slice = blockIdx.x; slice < n_slices; slice += gridDim.x) {
    const int k = slice * SWEEP_THREADS + tid;
    const double tt = text_th[min(k, K - 1)], dt = det_th[min(k, K - 1)];      // lanes past K work on a copy and add nothing
    long long acc[6] = {0, 0, 0, 0, 0, 0};
    for (int img = blockIdx.y; img < I; img += gridDim.y) {
      SweepImage s;
      if (!sweep_image(pair_off, gt_off, det_off, img, n_poly, n_gt, n_det, n_pairs, max_dets, s)) continue;
      int care_gt_e2e = 0, care_gt_det = 0;
      for (int g = 0; g < s.G; ++g) {
        care_gt_e2e += gt_dc_e2e[s.g0 + g] ? 0 : 1;
        care_gt_det += gt_dc_det[s.g0 + g] ? 0 : 1;
      }
      acc[1] += care_gt_e2e;
      acc[4] += care_gt_det;
      if (s.D == 0) continue;                                           // G == 0: nothing matches, the present detections still count
      const u64* grows = rows + s.row_off;
      const long long words = (long long)s.G * s.W;
      const bool in_lds = words <= GLASS_RRC_SWEEP_LDS_WORDS;              // uniform over the workgroup
      if (in_lds) {
        __syncthreads();                                                // the previous image's rows are no longer read
        for (int i = tid; i < (int)words; i += SWEEP_THREADS) lds_rows[i] = grows[i];
        __syncthreads();
      }
      if (s.W <= 1) {
        if (in_lds) SWEEP_LANE(1, lds_rows); else SWEEP_LANE(1, grows);
      } else if (s.W <= 2) {
        if (in_lds) SWEEP_LANE(2, lds_rows); else SWEEP_LANE(2, grows);
      } else if (s.W <= 4) {
        if (in_lds) SWEEP_LANE(4, lds_rows); else SWEEP_LANE(4, grows);
      } else if (s.W <= SWEEP_REG_WORDS) {
        if (in_lds) SWEEP_LANE(SWEEP_REG_WORDS, lds_rows); else SWEEP_LANE(SWEEP_REG_WORDS, grows);
      } else if (slot && s.W <= max_words) {
        sweep_lane_spill(in_lds ? (const u64*)lds_rows : grows, s, care_e2e, care_det, gt_dc_e2e, gt_dc_det, score_text, score_det,
                         gt_accept, det_word, tt, dt, acc, slot, max_words);
      }
    }
    if (k < K) {
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (acc[j]) atomicAdd(&counts[(long long)k * 6 + j], (u64)acc[j]);
    }
  }
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct SweepPlan {
  int gx, gy, max_words;
  int64_t row_words, care_words, spill_words;
};

SweepPlan sweep_plan(int n_images, int n_gt, int n_det, int64_t n_pairs, int max_dets, int n_comb) {
  SweepPlan p;
  p.max_words = (max_dets + 63) / 64;
  const bool spill = p.max_words > SWEEP_REG_WORDS;
  const int cap = spill ? SWEEP_MAX_BLOCKS_SPILL : SWEEP_MAX_BLOCKS;
  const int n_slices = cdiv(n_comb, SWEEP_THREADS);
  p.gx = n_slices < cap ? n_slices : cap;
  p.gy = cap / p.gx < n_images ? cap / p.gx : n_images;
  if (p.gy < 1) p.gy = 1;
  p.row_words = n_pairs / 64 + 2 * (int64_t)n_gt + 1;
  p.care_words = n_det / 64 + (int64_t)n_images + 1;
  p.spill_words = spill ? (int64_t)p.gx * p.gy * 2 * p.max_words * SWEEP_THREADS : 0;
  return p;
}

}  // namespace

extern "C" int64_t glass_rrc_sweep_workspace_bytes(int n_images, int n_gt, int n_det, int64_t n_pairs, int max_dets, int n_comb) {
  if (n_images <= 0 || n_gt < 0 || n_det < 0 || n_pairs < 0 || max_dets < 0 || n_comb < 1) return 0;
  const SweepPlan p = sweep_plan(n_images, n_gt, n_det, n_pairs, max_dets, n_comb);
  return align16(p.row_words * 8) + 2 * align16(p.care_words * 8) + align16(p.spill_words * 8);
}

extern "C" int glass_rrc_sweep(const double* area, int n_poly, const double* inter, int64_t n_pairs, const int64_t* pair_off,
                               const int* gt_off, const int* det_off, int n_images, const uint8_t* gt_dontcare_e2e,
                               const uint8_t* gt_dontcare_det, int n_gt, const uint8_t* det_dontcare_e2e,
                               const uint8_t* det_dontcare_det, const double* det_score_text, const double* det_score_det, int n_det,
                               int max_dets, const int* gt_accept, const int* det_word, const double* text_th, const double* det_th,
                               int n_comb, int64_t* counts, void* workspace, int64_t workspace_bytes, glass_stream_t stream) {
  GLASS_CHECK_ARG(n_comb >= 1 && n_comb <= GLASS_RRC_SWEEP_MAX_COMBINATIONS, "glass_rrc_sweep: %d combinations, must be 1 .. %d", n_comb,
                  GLASS_RRC_SWEEP_MAX_COMBINATIONS);
  GLASS_CHECK_ARG(n_poly >= 0 && n_pairs >= 0 && n_images >= 0 && n_gt >= 0 && n_det >= 0 && max_dets >= 0 && max_dets <= n_det &&
                      (int64_t)n_gt + n_det <= n_poly,
                  "glass_rrc_sweep: bad sizes n_poly=%d n_pairs=%lld n_images=%d n_gt=%d n_det=%d max_dets=%d", n_poly, (long long)n_pairs,
                  n_images, n_gt, n_det, max_dets);
  GLASS_CHECK_ARG(text_th && det_th && counts, "glass_rrc_sweep: null thresholds or counts");
  if (n_images == 0 || (n_gt == 0 && n_det == 0)) return GLASS_OK;
  GLASS_CHECK_ARG(area && pair_off && gt_off && det_off && workspace, "glass_rrc_sweep: null pointer");
  GLASS_CHECK_ARG(n_gt == 0 || (gt_dontcare_e2e && gt_dontcare_det && gt_accept), "glass_rrc_sweep: null GT array");
  GLASS_CHECK_ARG(n_det == 0 || (det_dontcare_e2e && det_dontcare_det && det_score_text && det_score_det && det_word),
                  "glass_rrc_sweep: null detection array");
  GLASS_CHECK_ARG(n_pairs == 0 || inter, "glass_rrc_sweep: null inter");
  GLASS_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)gt_accept & 15) == 0,
                  "glass_rrc_sweep: workspace and gt_accept must be 16-byte aligned");
  GLASS_CHECK_ARG(workspace_bytes >= glass_rrc_sweep_workspace_bytes(n_images, n_gt, n_det, n_pairs, max_dets, n_comb),
                  "glass_rrc_sweep: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
                  (long long)glass_rrc_sweep_workspace_bytes(n_images, n_gt, n_det, n_pairs, max_dets, n_comb));
  const SweepPlan p = sweep_plan(n_images, n_gt, n_det, n_pairs, max_dets, n_comb);
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  u64* rows = reinterpret_cast<u64*>(ws);
  u64* care_e2e = reinterpret_cast<u64*>(ws + align16(p.row_words * 8));
  u64* care_det = reinterpret_cast<u64*>(ws + align16(p.row_words * 8) + align16(p.care_words * 8));
  u64* spill = p.spill_words ? reinterpret_cast<u64*>(ws + align16(p.row_words * 8) + 2 * align16(p.care_words * 8)) : nullptr;
  hipLaunchKernelGGL(rrc_sweep_bits_kernel, dim3((unsigned)(n_images < 65536 ? n_images : 65536)), dim3(SWEEP_THREADS), 0, st, area,
                     n_poly, inter, (long long)n_pairs, reinterpret_cast<const long long*>(pair_off), gt_off, det_off, n_images, n_gt,
                     n_det, max_dets, det_dontcare_e2e, det_dontcare_det, rows, care_e2e, care_det);
  GLASS_CHECK_LAUNCH("glass_rrc_sweep (bits)");
  hipLaunchKernelGGL(rrc_sweep_kernel, dim3((unsigned)p.gx, (unsigned)p.gy), dim3(SWEEP_THREADS), 0, st, n_poly, (long long)n_pairs,
                     reinterpret_cast<const long long*>(pair_off), gt_off, det_off, n_images, gt_dontcare_e2e, gt_dontcare_det, n_gt,
                     n_det, max_dets, det_score_text, det_score_det, gt_accept, det_word, text_th, det_th, n_comb, rows, care_e2e,
                     care_det, spill, p.max_words, reinterpret_cast<u64*>(counts));
  GLASS_CHECK_LAUNCH("glass_rrc_sweep");
  return GLASS_OK;
}
