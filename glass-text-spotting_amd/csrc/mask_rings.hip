// Mask polygonisation (reference glass/evaluation/text_evaluator.py:464-492, `masks_to_polygons`): the largest 4-connected
// region of every mask of a uint8 / bool [R][H][W] tensor as its exterior ring on the pixel-corner lattice, with exactly the
// semantics of the host tracer glass_amd.evaluation.masks_to_polygons (start at the top-left corner of the region's first
// raster pixel, head east, region on the right-hand side, a vertex only where the boundary turns, right turn at a diagonal
// pinch, closed ring).
//
// Stages (every one after the first touches only the window of a mask, i.e. the tight rectangle of its set pixels):
//   window   one streaming pass over [R][H][W], 16-byte loads, min / max of the set pixels' rows and columns per mask
//            (integer atomicMin / atomicMax: order-free).
//   offsets  one workgroup: running sum of the window areas -> where each mask's labels live in the workspace.
//   label    union-find on the window, one wavefront per 64 pixels of a row: a pixel starts as the first pixel of its
//            horizontal run (a ballot), runs are united with the run left of the 64-column seam and with the runs above
//            (one union per overlap), atomicMin on the roots.  A label only ever decreases, so a root is the SMALLEST linear
//            index of its region = its first raster pixel, whatever the order of the atomics: nothing visible depends on
//            scheduling.  Then every pixel is pointed at its root and the pixels of each root are counted (one atomicAdd per
//            run), and the winner is the maximum of (count << 32 | ~root): most pixels, then first raster pixel.
//   trace    one workgroup per mask: the winner's window as a bitmap in LDS (a bit per pixel) when it fits in
//            GLASS_MASK_RINGS_LDS_WORDS 64-bit words, else straight from the labels in global memory; wavefront 0 walks the
//            ring, lane l looking at the corner l + 1 edges ahead, so a straight run costs one ballot per 64 edges and every
//            iteration ends at a turn.  Run twice: once counting the vertices (-> ring_off by a running sum), once writing.
// Every loop is bounded by a size read once: a parent chain strictly decreases, a union lowers one of its two ends every
// turn, the walk is cut at the number of directed boundary edges of the window (status 3 if that ever happens).  No wait
// on another workgroup.
//
// RoI form (glass_roi_mask_windows / glass_roi_mask_rings_count, include/glass_hip_feature_roimask.h): the pasted [R][H][W]
// tensor never exists.  Whether a pixel is set is the paste's own arithmetic (paste_value of mask_paste_common.h) >= the
// threshold, evaluated from the M x M RoI mask and its box in the two stages that read pixels: the window stage, over the
// box's candidate rectangle (paste_rect: clipped to the image before it is an integer) instead of the whole image, and the
// first labelling stage.  The windows are the same tight ones, so the workspace, the labels, the winners and the rings are
// those of the byte form on the pasted tensor, bit for bit; every later stage is shared.
#include <climits>
#include "common.h"
#include "glass_hip_feature_roimask.h"
#include "mask_paste_common.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_WAVES = MR_THREADS / 64;
constexpr int MR_LDS_WORDS = GLASS_MASK_RINGS_LDS_WORDS;
constexpr long MR_BYTES_PER_BLOCK = 65536;           // window pass: bytes of one mask streamed by one workgroup at a time
constexpr int MR_MAX_GRID_X = 1024;
constexpr int MR_LABEL_GRID_X = 64;                  // label kernels: 256 wavefronts stride over the rows of one window

enum { MR_OK = 0, MR_SHORT_WORKSPACE = 2, MR_WALK_BOUND = 3, MR_TOO_MANY_POINTS = 4 };

struct Window {
  int x0, y0, w, h;
};

// a window that leaves the image, or is inverted, is an empty mask (glass_mask_windows writes x1 < x0 for an empty mask)
__device__ __host__ inline Window window_of(const int* win4, int H, int W) {
  Window q = {0, 0, 0, 0};
  const int x0 = win4[0], y0 = win4[1], x1 = win4[2], y1 = win4[3];
  if (x0 < 0 || y0 < 0 || x1 >= W || y1 >= H || x1 < x0 || y1 < y0) return q;
  q.x0 = x0;
  q.y0 = y0;
  q.w = x1 - x0 + 1;
  q.h = y1 - y0 + 1;
  return q;
}

__global__ void mr_window_init_kernel(int4* __restrict__ win, int R, int H, int W) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) win[r] = make_int4(W, H, -1, -1);
}

__device__ __forceinline__ void mr_note(long idx, int W, int& xlo, int& ylo, int& xhi, int& yhi) {
  const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
  xlo = min(xlo, x);
  xhi = max(xhi, x);
  ylo = min(ylo, y);
  yhi = max(yhi, y);
}

// the workgroup's extremes of one mask -> its window (integer atomicMin / atomicMax); called by every thread, once per mask.
// For the RoI form's window stage: the reduction mr_window_kernel ends with, which stays written out there so that the
// byte form's code is what it was (called from there, force-inlined, this helper compiles to 3370 instructions for that
// kernel instead of 3366, whether it takes the LDS array by pointer or by reference).
__device__ __forceinline__ void mr_window_reduce(int xlo, int ylo, int xhi, int yhi, int (&red)[MR_WAVES][4], int* __restrict__ win, int r) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    xlo = min(xlo, __shfl_xor(xlo, off));
    ylo = min(ylo, __shfl_xor(ylo, off));
    xhi = max(xhi, __shfl_xor(xhi, off));
    yhi = max(yhi, __shfl_xor(yhi, off));
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = xlo;
    red[tid >> 6][1] = ylo;
    red[tid >> 6][2] = xhi;
    red[tid >> 6][3] = yhi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < MR_WAVES; ++k) {
      xlo = min(xlo, red[k][0]);
      ylo = min(ylo, red[k][1]);
      xhi = max(xhi, red[k][2]);
      yhi = max(yhi, red[k][3]);
    }
    if (xhi >= 0) {
      atomicMin(&win[4 * r + 0], xlo);
      atomicMin(&win[4 * r + 1], ylo);
      atomicMax(&win[4 * r + 2], xhi);
      atomicMax(&win[4 * r + 3], yhi);
    }
  }
  __syncthreads();
}

// grid (chunks of a mask, masks); a mask is a flat run of H * W bytes: the bytes before the first 16-byte boundary and
// after the last one are read one by one by the first workgroup, everything between as uint4
__global__ __launch_bounds__(MR_THREADS) void mr_window_kernel(const unsigned char* __restrict__ masks, int R, int H, int W,
                                                               int* __restrict__ win) {
  const long HW = (long)H * W;
  const int tid = threadIdx.x;
  __shared__ int red[MR_WAVES][4];
  for (int r = blockIdx.y; r < R; r += gridDim.y) {                    // uniform over the workgroup
    const unsigned char* m = masks + (size_t)r * HW;
    const long head = min(HW, (long)((16 - ((uintptr_t)m & 15)) & 15));
    const long nvec = (HW - head) / 16;
    const long tail = head + nvec * 16;
    int xlo = INT_MAX, ylo = INT_MAX, xhi = -1, yhi = -1;
    const long per_block = MR_BYTES_PER_BLOCK / 16;
    for (long c = blockIdx.x; c * per_block < nvec; c += gridDim.x) {
      const long vend = min(nvec, (c + 1) * per_block);
      for (long v = c * per_block + tid; v < vend; v += MR_THREADS) {
        const uint4 q = *reinterpret_cast<const uint4*>(m + head + v * 16);
        if (q.x | q.y | q.z | q.w) {
          const unsigned int wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!wds[k]) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if ((wds[k] >> (8 * b)) & 0xffu) mr_note(head + v * 16 + k * 4 + b, W, xlo, ylo, xhi, yhi);
          }
        }
      }
    }
    if (blockIdx.x == 0 && tid < 16) {
      if (tid < head && m[tid]) mr_note(tid, W, xlo, ylo, xhi, yhi);
      if (tail + tid < HW && m[tail + tid]) mr_note(tail + tid, W, xlo, ylo, xhi, yhi);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      xlo = min(xlo, __shfl_xor(xlo, off));
      ylo = min(ylo, __shfl_xor(ylo, off));
      xhi = max(xhi, __shfl_xor(xhi, off));
      yhi = max(yhi, __shfl_xor(yhi, off));
    }
    if ((tid & 63) == 0) {
      red[tid >> 6][0] = xlo;
      red[tid >> 6][1] = ylo;
      red[tid >> 6][2] = xhi;
      red[tid >> 6][3] = yhi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < MR_WAVES; ++k) {
        xlo = min(xlo, red[k][0]);
        ylo = min(ylo, red[k][1]);
        xhi = max(xhi, red[k][2]);
        yhi = max(yhi, red[k][3]);
      }
      if (xhi >= 0) {
        atomicMin(&win[4 * r + 0], xlo);
        atomicMin(&win[4 * r + 1], ylo);
        atomicMax(&win[4 * r + 2], xhi);
        atomicMax(&win[4 * r + 3], yhi);
      }
    }
    __syncthreads();
  }
}

// RoI form of the window stage, grid (workgroups over a rectangle, masks): the set pixels are looked for in the box's
// candidate rectangle only.  The loop runs over the clipped rectangle's pixel count, read once.
__global__ __launch_bounds__(MR_THREADS) void mr_roi_window_kernel(const float* __restrict__ masks, const float* __restrict__ boxes,
                                                                   int R, int M, int H, int W, float threshold,
                                                                   int* __restrict__ win) {
  const int tid = threadIdx.x;
  __shared__ int red[MR_WAVES][4];
  for (int r = blockIdx.y; r < R; r += gridDim.y) {                    // uniform over the workgroup
    const int4 rc = paste_rect(boxes + (size_t)r * 5, M, H, W);
    if (rc.z < rc.x) continue;                                         // nothing can be set: the window stays empty
    const int rw = rc.z - rc.x + 1, rh = rc.w - rc.y + 1;
    const long long npx = (long long)rw * rh;
    const PasteFrame f = paste_frame(boxes + (size_t)r * 5, M);
    const float* mk = masks + (size_t)r * M * M;
    int xlo = INT_MAX, ylo = INT_MAX, xhi = -1, yhi = -1;
    for (long long i = (long long)blockIdx.x * MR_THREADS + tid; i < npx; i += (long long)gridDim.x * MR_THREADS) {
      const int y = (int)(i / rw), x = (int)(i - (long long)y * rw);
      const int px = rc.x + x, py = rc.y + y;
      if (paste_value(f, mk, M, px, py) >= threshold) {
        xlo = min(xlo, px);
        xhi = max(xhi, px);
        ylo = min(ylo, py);
        yhi = max(yhi, py);
      }
    }
    mr_window_reduce(xlo, ylo, xhi, yhi, red, win, r);
  }
}

// the candidate rectangles themselves, for whoever wants to see what the window stage looked at
__global__ void mr_roi_rect_kernel(const float* __restrict__ boxes, int R, int M, int H, int W, int4* __restrict__ rects) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < R) rects[r] = paste_rect(boxes + (size_t)r * 5, M, H, W);
}

// one workgroup: out[0] = 0, out[k + 1] = out[k] + value(k), *total = out[n]; every thread sums a contiguous slice and the
// slice totals are scanned in LDS by thread 0
template <typename Out, typename Value>
__device__ void mr_block_scan(int n, Out* __restrict__ out, Value value, long long* part, long long* total) {
  const int tid = threadIdx.x;
  const int per = (n + MR_THREADS - 1) / MR_THREADS;
  const int b = (int)min((long)n, (long)tid * per), e = (int)min((long)n, (long)b + per);
  long long s = 0;
  for (int k = b; k < e; ++k) s += value(k);
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int k = 0; k < MR_THREADS; ++k) {
      const long long v = part[k];
      part[k] = run;
      run += v;
    }
    *total = run;
  }
  __syncthreads();
  s = part[tid];
  for (int k = b; k < e; ++k) {
    out[k] = (Out)s;
    s += value(k);
  }
  if (tid == 0) out[n] = (Out)*total;
}

__global__ __launch_bounds__(MR_THREADS) void mr_offsets_kernel(const int* __restrict__ win, int R, int H, int W,
                                                                long long cap_px, long long* __restrict__ pix_off,
                                                                unsigned long long* __restrict__ best, int* __restrict__ nvert,
                                                                int* __restrict__ status) {
  __shared__ long long part[MR_THREADS];
  __shared__ long long total;
  mr_block_scan(R, pix_off, [&](int k) {
    const Window q = window_of(win + 4 * k, H, W);
    return (long long)q.w * q.h;
  }, part, &total);
  for (int r = threadIdx.x; r < R; r += MR_THREADS) {
    best[r] = 0ull;
    nvert[r] = 0;
  }
  if (threadIdx.x == 0) *status = total > cap_px ? MR_SHORT_WORKSPACE : MR_OK;
}

__device__ __forceinline__ int mr_load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// the root of a: a label never exceeds its index, so the chain strictly decreases and ends within a + 1 steps
__device__ __forceinline__ int mr_find(const int* L, int a) {
  for (;;) {
    const int p = mr_load(L + a);
    if (p >= a || p < 0) return a;
    a = p;
  }
}

// unite the regions of a and b: hang the larger root under the smaller one.  A turn either ends or lowers a or b.
__device__ __forceinline__ void mr_union(int* L, int a, int b, long long bound) {
  for (long long it = 0; it < bound; ++it) {
    a = mr_find(L, a);
    b = mr_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

enum { MR_INIT = 0, MR_MERGE = 1, MR_COUNT = 2, MR_SELECT = 3 };

// MR_INIT for the 64 pixels of one wavefront, whatever told it which are set: a set pixel starts as the first pixel of its run
__device__ __forceinline__ void mr_init_labels(bool in, bool set, int lane, unsigned long long below, int p, int* L, int* C) {
  const unsigned long long bal = __ballot(set);
  const unsigned long long gaps = ~bal & below;                 // unset lanes below this one
  const int start = gaps ? 64 - __clzll((long long)gaps) : 0;   // first lane of this lane's run
  if (in) {
    L[p] = set ? p - (lane - start) : -1;
    C[p] = 0;
  }
}

// grid (wavefront groups, masks): wavefront `it` of a mask owns the 64 pixels (y, xs .. xs + 63) of its window
template <int STAGE>
__global__ __launch_bounds__(MR_THREADS) void mr_label_kernel(const unsigned char* __restrict__ masks, int R, int H, int W,
                                                              const int* __restrict__ win, const long long* __restrict__ pix_off,
                                                              int* labels, int* cnt, unsigned long long* best,
                                                              const int* __restrict__ status) {
  if (*status != MR_OK) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const Window q = window_of(win + 4 * r, H, W);
    if (q.w == 0) continue;
    const int segs = (q.w + 63) / 64;
    const long long items = (long long)q.h * segs;
    const long long npix = (long long)q.w * q.h;
    int* L = labels + pix_off[r];
    int* C = cnt + pix_off[r];
    const unsigned char* m = STAGE == MR_INIT ? masks + (size_t)r * H * W + (size_t)q.y0 * W + q.x0 : nullptr;   // read by MR_INIT only
    for (long long it = (long long)blockIdx.x * MR_WAVES + wid; it < items; it += (long long)gridDim.x * MR_WAVES) {
      const int y = (int)(it / segs);
      const int xs = (int)(it - (long long)y * segs) * 64;
      const int x = xs + lane;
      const bool in = x < q.w;
      const int p = y * q.w + x;
      if (STAGE == MR_INIT) {
        mr_init_labels(in, in && m[(size_t)y * W + x] != 0, lane, below, p, L, C);
      } else if (STAGE == MR_MERGE) {
        const bool set = in && mr_load(L + p) >= 0;                    // the sign of a label never changes after MR_INIT
        const unsigned long long bal = __ballot(set);
        if (set) {
          const bool left = lane ? ((bal >> (lane - 1)) & 1ull) != 0 : (x > 0 && mr_load(L + p - 1) >= 0);
          if (lane == 0 && left) mr_union(L, p, p - 1, 2 * npix + 2);  // the run goes on across the 64-column seam
          if (y > 0 && mr_load(L + p - q.w) >= 0) {
            // one union per overlap of this run with a run above: at the overlap's first column
            const bool upleft = x > 0 && mr_load(L + p - q.w - 1) >= 0;
            if (!left || !upleft) mr_union(L, p, p - q.w, 2 * npix + 2);
          }
        }
      } else if (STAGE == MR_COUNT) {
        const bool set = in && mr_load(L + p) >= 0;
        const unsigned long long bal = __ballot(set);
        if (set) {
          const int root = mr_find(L, p);
          L[p] = root;                                                 // still an ancestor for whoever passes through p
          if (lane == 0 || !((bal >> (lane - 1)) & 1ull)) {            // first lane of a run: all of it has this root
            const unsigned long long rest = ~bal >> lane;              // the run ends at the first unset lane from here
            const int len = rest ? __ffsll((long long)rest) - 1 : 64 - lane;
            atomicAdd(C + root, len);
          }
        }
      } else {
        unsigned long long key = 0ull;
        if (in && L[p] == p) key = ((unsigned long long)(unsigned)C[p] << 32) | (0xffffffffu - (unsigned)p);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long o = __shfl_xor(key, off);
          key = o > key ? o : key;
        }
        if (lane == 0 && key) atomicMax(best + r, key);
      }
    }
  }
}

// MR_INIT of the RoI form, same grid and the same walk over the window as mr_label_kernel: a pixel is set iff the paste's
// value there reaches the threshold.  The window lies inside the image (window_of), the mask taps inside [M][M] (paste_value).
__global__ __launch_bounds__(MR_THREADS) void mr_roi_label_init_kernel(const float* __restrict__ masks, const float* __restrict__ boxes,
                                                                       int R, int M, int H, int W, float threshold,
                                                                       const int* __restrict__ win,
                                                                       const long long* __restrict__ pix_off, int* labels, int* cnt,
                                                                       const int* __restrict__ status) {
  if (*status != MR_OK) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int r = blockIdx.y; r < R; r += gridDim.y) {
    const Window q = window_of(win + 4 * r, H, W);
    if (q.w == 0) continue;
    const int segs = (q.w + 63) / 64;
    const long long items = (long long)q.h * segs;
    int* L = labels + pix_off[r];
    int* C = cnt + pix_off[r];
    const PasteFrame f = paste_frame(boxes + (size_t)r * 5, M);
    const float* mk = masks + (size_t)r * M * M;
    for (long long it = (long long)blockIdx.x * MR_WAVES + wid; it < items; it += (long long)gridDim.x * MR_WAVES) {
      const int y = (int)(it / segs);
      const int xs = (int)(it - (long long)y * segs) * 64;
      const int x = xs + lane;
      const bool in = x < q.w;
      const bool set = in && paste_value(f, mk, M, q.x0 + x, q.y0 + y) >= threshold;
      mr_init_labels(in, set, lane, below, y * q.w + x, L, C);
    }
  }
}

// is pixel (y, x) of the window part of the winner?  LDS: the bitmap; otherwise the labels (every pixel points at its root)
template <bool LDS>
__device__ __forceinline__ bool mr_pix(const unsigned long long* bm, const int* L, int root, int w, int h, int nw, int y, int x) {
  if (y < 0 || y >= h || x < 0 || x >= w) return false;
  if (LDS) return (bm[y * nw + (x >> 6)] >> (x & 63)) & 1ull;
  return L[(long long)y * w + x] == root;
}

// wavefront 0: the ring of the winner (root = its first raster pixel).  Returns the number of vertices, -1 if the walk did
// not close within the number of directed boundary edges of the window.  WRITE: vertices go to xy[0 .. cap), image coordinates.
template <bool LDS, bool WRITE>
__device__ int mr_walk(const unsigned long long* bm, const int* L, int root, const Window q, int nw, int2* xy, int cap) {
  const int lane = threadIdx.x & 63;
  const int ry = root / q.w, rx = root - ry * q.w;
  int y = ry, x = rx, d = 0, n = 0;                                    // corner (y, x); 0 E, 1 S, 2 W, 3 N
  if (WRITE && lane == 0 && n < cap) xy[n] = make_int2(x + q.x0, y + q.y0);
  ++n;
  const long long bound = 2 * ((long long)(q.w + 1) * q.h + (long long)(q.h + 1) * q.w) + 4;
  for (long long it = 0; it < bound; ++it) {
    const int dx = d == 0 ? 1 : (d == 2 ? -1 : 0), dy = d == 1 ? 1 : (d == 3 ? -1 : 0);
    // the pixel ahead of a corner on the right / left hand side, relative to the corner: SE (0,0) SW (0,-1) NW (-1,-1) NE (-1,0)
    const int ryo = d >= 2 ? -1 : 0, rxo = (d == 1 || d == 2) ? -1 : 0;
    const int lyo = (d == 0 || d == 3) ? -1 : 0, lxo = d >= 2 ? -1 : 0;
    const int cy = y + (lane + 1) * dy, cx = x + (lane + 1) * dx;      // the corner lane + 1 edges ahead
    const bool right = mr_pix<LDS>(bm, L, root, q.w, q.h, nw, cy + ryo, cx + rxo);
    const bool left = mr_pix<LDS>(bm, L, root, q.w, q.h, nw, cy + lyo, cx + lxo);
    const unsigned long long straight = __ballot(right && !left);
    const unsigned long long rb = __ballot(right);
    if (straight == ~0ull) {
      y += 64 * dy;
      x += 64 * dx;
      continue;
    }
    const int t = __ffsll((long long)~straight) - 1;                   // the first corner where the boundary turns
    y += (t + 1) * dy;
    x += (t + 1) * dx;
    d = ((rb >> t) & 1ull) ? (d + 3) & 3 : (d + 1) & 3;                // blocked ahead: left; region ends: right (also at a pinch)
    if (WRITE && lane == 0 && n < cap) xy[n] = make_int2(x + q.x0, y + q.y0);
    ++n;
    if (y == ry && x == rx && d == 0) return n;
    if (n == INT_MAX) return -1;
  }
  return -1;
}

template <bool WRITE>
__global__ __launch_bounds__(MR_THREADS) void mr_trace_kernel(int R, int H, int W, const int* __restrict__ win,
                                                              const long long* __restrict__ pix_off, long long cap_px,
                                                              const int* __restrict__ labels,
                                                              const unsigned long long* __restrict__ best, int* nvert,
                                                              const int* __restrict__ ring_off, int2* xy, long long n_points,
                                                              int* status) {
  __shared__ unsigned long long bm[MR_LDS_WORDS];
  if (*status != MR_OK) return;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {                    // uniform over the workgroup
    const Window q = window_of(win + 4 * r, H, W);
    const unsigned long long key = best[r];
    if (q.w == 0 || key == 0ull) continue;                             // empty mask: no vertex
    const long long npix = (long long)q.w * q.h, po = pix_off[r];
    const long long root64 = 0xffffffffll - (long long)(key & 0xffffffffull);
    if (root64 >= npix || po < 0 || po + npix > cap_px) continue;      // not a workspace of glass_mask_rings_count
    const int root = (int)root64;
    const int* L = labels + po;
    const int nw = (q.w + 63) / 64;
    const bool lds = (long long)nw * q.h <= MR_LDS_WORDS;
    if (lds) {
      const int items = nw * q.h;
      for (int it = wid; it < items; it += MR_WAVES) {
        const int y = it / nw, x = (it - y * nw) * 64 + lane;
        const unsigned long long bits = __ballot(x < q.w && L[y * q.w + x] == root);
        if (lane == 0) bm[it] = bits;
      }
    }
    __syncthreads();
    if (wid == 0) {
      int2* out = nullptr;
      int cap = 0;
      if (WRITE) {
        const long long b = ring_off[r], e = ring_off[r + 1];
        if (b >= 0 && e >= b && e <= n_points) {
          out = xy + b;
          cap = (int)(e - b);
        }
      }
      const int n = lds ? mr_walk<true, WRITE>(bm, L, root, q, nw, out, cap) : mr_walk<false, WRITE>(bm, L, root, q, nw, out, cap);
      if (lane == 0) {
        if (n < 0 || (WRITE && n != cap)) *status = MR_WALK_BOUND;
        else if (!WRITE) nvert[r] = n;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(MR_THREADS) void mr_ring_offsets_kernel(const int* __restrict__ nvert, int R, int* __restrict__ ring_off,
                                                                     int* status) {
  __shared__ long long part[MR_THREADS];
  __shared__ long long total;
  if (*status != MR_OK) {                                              // no ring is reported from a failed run
    for (int r = threadIdx.x; r <= R; r += MR_THREADS) ring_off[r] = 0;
    return;
  }
  mr_block_scan(R, ring_off, [&](int k) { return (long long)nvert[k]; }, part, &total);
  if (threadIdx.x == 0 && total > INT_MAX) {
    *status = MR_TOO_MANY_POINTS;
    ring_off[R] = 0;
  }
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// workspace: pix_off int64 [R + 1] | best uint64 [R] | nvert int32 [R] | labels int32 [cap_px] | counts int32 [cap_px]
struct Layout {
  int64_t best, nvert, labels;
};
Layout layout_of(int R) {
  Layout l;
  l.best = align16((int64_t)(R + 1) * 8);
  l.nvert = l.best + align16((int64_t)R * 8);
  l.labels = l.nvert + align16((int64_t)R * 4);
  return l;
}
long long cap_px_of(int64_t workspace_bytes, const Layout& l) { return (workspace_bytes - l.labels) / 32 * 4; }

bool sizes_ok(int R, int H, int W) { return R >= 0 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && (int64_t)H * W <= INT_MAX; }

unsigned grid_masks(int R) { return (unsigned)(R < 65535 ? R : 65535); }

// GLASS_CHECK_LAUNCH with the entry point's name and the stage in the message
#define MR_CHECK_LAUNCH(what, stage)                                                          \
  do {                                                                                        \
    hipError_t e__ = hipGetLastError();                                                       \
    if (e__ != hipSuccess) {                                                                  \
      glass_set_error("%s (%s): launch failed: %s", what, stage, hipGetErrorString(e__));     \
      return GLASS_EHIP;                                                                      \
    }                                                                                         \
  } while (0)

// the count after the form's own argument checks: offsets, the four labelling stages (`init` enqueues the first, the only
// one that looks at pixels), the counting walk and the ring offsets
template <typename Init>
int rings_count(const char* what, int R, int H, int W, const int* windows, void* workspace, int64_t workspace_bytes, int* ring_off,
                int* status, hipStream_t st, Init init) {
  GLASS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", what);
  const Layout l = layout_of(R);
  GLASS_CHECK_ARG(workspace_bytes >= l.labels, "%s: workspace of %lld bytes, needs %lld and the windows", what,
                  (long long)workspace_bytes, (long long)l.labels);
  const long long cap_px = cap_px_of(workspace_bytes, l);
  char* ws = static_cast<char*>(workspace);
  long long* pix_off = reinterpret_cast<long long*>(ws);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + l.best);
  int* nvert = reinterpret_cast<int*>(ws + l.nvert);
  int* labels = reinterpret_cast<int*>(ws + l.labels);
  int* cnt = labels + cap_px;
  const unsigned char* none = nullptr;                                 // the later stages read labels only
  hipLaunchKernelGGL(mr_offsets_kernel, dim3(1), dim3(MR_THREADS), 0, st, windows, R, H, W, cap_px, pix_off, best, nvert, status);
  MR_CHECK_LAUNCH(what, "offsets");
  const dim3 g(MR_LABEL_GRID_X, grid_masks(R));
  init(g, st, pix_off, labels, cnt, best);
  hipLaunchKernelGGL(mr_label_kernel<MR_MERGE>, g, dim3(MR_THREADS), 0, st, none, R, H, W, windows, pix_off, labels, cnt, best, status);
  hipLaunchKernelGGL(mr_label_kernel<MR_COUNT>, g, dim3(MR_THREADS), 0, st, none, R, H, W, windows, pix_off, labels, cnt, best, status);
  hipLaunchKernelGGL(mr_label_kernel<MR_SELECT>, g, dim3(MR_THREADS), 0, st, none, R, H, W, windows, pix_off, labels, cnt, best, status);
  MR_CHECK_LAUNCH(what, "label");
  hipLaunchKernelGGL(mr_trace_kernel<false>, dim3(grid_masks(R)), dim3(MR_THREADS), 0, st, R, H, W, windows, pix_off, cap_px, labels, best,
                     nvert, (const int*)nullptr, (int2*)nullptr, 0ll, status);
  MR_CHECK_LAUNCH(what, "trace");
  hipLaunchKernelGGL(mr_ring_offsets_kernel, dim3(1), dim3(MR_THREADS), 0, st, nvert, R, ring_off, status);
  MR_CHECK_LAUNCH(what, "ring offsets");
  return GLASS_OK;
}

}  // namespace

extern "C" int glass_mask_windows(const uint8_t* masks, int R, int H, int W, int* windows, glass_stream_t stream) {
  GLASS_CHECK_ARG(sizes_ok(R, H, W), "glass_mask_windows: bad sizes R=%d H=%d W=%d (H, W in 1..65535, H * W < 2^31)", R, H, W);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(masks && windows, "glass_mask_windows: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)windows & 15) == 0, "glass_mask_windows: windows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mr_window_init_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, reinterpret_cast<int4*>(windows), R, H, W);
  GLASS_CHECK_LAUNCH("glass_mask_windows (init)");
  const long chunks = ((long)H * W + MR_BYTES_PER_BLOCK - 1) / MR_BYTES_PER_BLOCK;
  hipLaunchKernelGGL(mr_window_kernel, dim3((unsigned)(chunks < MR_MAX_GRID_X ? chunks : MR_MAX_GRID_X), grid_masks(R)), dim3(MR_THREADS),
                     0, st, masks, R, H, W, windows);
  GLASS_CHECK_LAUNCH("glass_mask_windows");
  return GLASS_OK;
}

extern "C" int64_t glass_mask_rings_workspace_bytes(const int* windows_host, int R, int H, int W) {
  if (R <= 0 || !windows_host || !sizes_ok(R, H, W)) return 0;
  int64_t px = 0;
  for (int r = 0; r < R; ++r) {
    const Window q = window_of(windows_host + 4 * r, H, W);
    px += (int64_t)q.w * q.h;
  }
  return layout_of(R).labels + 2 * align16(px * 4);
}

extern "C" int glass_mask_rings_count(const uint8_t* masks, int R, int H, int W, const int* windows, void* workspace,
                                      int64_t workspace_bytes, int* ring_off, int* status, glass_stream_t stream) {
  GLASS_CHECK_ARG(sizes_ok(R, H, W), "glass_mask_rings_count: bad sizes R=%d H=%d W=%d (H, W in 1..65535, H * W < 2^31)", R, H, W);
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(masks && windows && workspace && ring_off && status, "glass_mask_rings_count: null pointer");
  return rings_count("glass_mask_rings_count", R, H, W, windows, workspace, workspace_bytes, ring_off, status, (hipStream_t)stream,
                     [&](dim3 g, hipStream_t st, const long long* pix_off, int* labels, int* cnt, unsigned long long* best) {
                       hipLaunchKernelGGL(mr_label_kernel<MR_INIT>, g, dim3(MR_THREADS), 0, st, masks, R, H, W, windows, pix_off, labels,
                                          cnt, best, status);
                     });
}

extern "C" int glass_mask_rings_write(int R, int H, int W, const int* windows, const void* workspace, int64_t workspace_bytes,
                                      const int* ring_off, int* xy, int64_t n_points, int* status, glass_stream_t stream) {
  GLASS_CHECK_ARG(sizes_ok(R, H, W), "glass_mask_rings_write: bad sizes R=%d H=%d W=%d (H, W in 1..65535, H * W < 2^31)", R, H, W);
  GLASS_CHECK_ARG(n_points >= 0 && n_points <= INT_MAX, "glass_mask_rings_write: n_points=%lld", (long long)n_points);
  if (R == 0 || n_points == 0) return GLASS_OK;
  GLASS_CHECK_ARG(windows && workspace && ring_off && xy && status, "glass_mask_rings_write: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)xy & 7) == 0,
                  "glass_mask_rings_write: workspace must be 16-byte and xy 8-byte aligned");
  const Layout l = layout_of(R);
  GLASS_CHECK_ARG(workspace_bytes >= l.labels, "glass_mask_rings_write: workspace of %lld bytes, needs %lld and the windows",
                  (long long)workspace_bytes, (long long)l.labels);
  const char* ws = static_cast<const char*>(workspace);
  hipLaunchKernelGGL(mr_trace_kernel<true>, dim3(grid_masks(R)), dim3(MR_THREADS), 0, (hipStream_t)stream, R, H, W, windows,
                     reinterpret_cast<const long long*>(ws), cap_px_of(workspace_bytes, l), reinterpret_cast<const int*>(ws + l.labels),
                     reinterpret_cast<const unsigned long long*>(ws + l.best), (int*)nullptr, ring_off, reinterpret_cast<int2*>(xy),
                     (long long)n_points, status);
  GLASS_CHECK_LAUNCH("glass_mask_rings_write");
  return GLASS_OK;
}

// ---------------------------------------------------------------------------------------------------------- RoI form

namespace {

int roi_args_ok(const char* what, int R, int M, int H, int W, float threshold) {
  GLASS_CHECK_ARG(sizes_ok(R, H, W), "%s: bad sizes R=%d H=%d W=%d (H, W in 1..65535, H * W < 2^31)", what, R, H, W);
  GLASS_CHECK_ARG(M >= 1 && M <= 4096, "%s: M=%d (1..4096)", what, M);
  GLASS_CHECK_ARG(threshold > 0.f, "%s: threshold=%g must be positive (at 0 or below the paste sets the whole image, or is the "
                  "visualisation mode)", what, (double)threshold);
  return GLASS_OK;
}

}  // namespace

extern "C" int glass_roi_mask_rects(const float* boxes, int R, int M, int H, int W, int* rects, glass_stream_t stream) {
  if (int rc = roi_args_ok("glass_roi_mask_rects", R, M, H, W, 1.f)) return rc;
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(boxes && rects, "glass_roi_mask_rects: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)rects & 15) == 0, "glass_roi_mask_rects: rects must be 16-byte aligned");
  hipLaunchKernelGGL(mr_roi_rect_kernel, dim3(cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, boxes, R, M, H, W,
                     reinterpret_cast<int4*>(rects));
  GLASS_CHECK_LAUNCH("glass_roi_mask_rects");
  return GLASS_OK;
}

extern "C" int glass_roi_mask_windows(const float* masks, const float* boxes, int R, int M, int H, int W, float threshold,
                                      int* windows, glass_stream_t stream) {
  if (int rc = roi_args_ok("glass_roi_mask_windows", R, M, H, W, threshold)) return rc;
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(masks && boxes && windows, "glass_roi_mask_windows: null pointer");
  GLASS_CHECK_ARG(((uintptr_t)windows & 15) == 0, "glass_roi_mask_windows: windows must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mr_window_init_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, reinterpret_cast<int4*>(windows), R, H, W);
  GLASS_CHECK_LAUNCH("glass_roi_mask_windows (init)");
  hipLaunchKernelGGL(mr_roi_window_kernel, dim3(MR_LABEL_GRID_X, grid_masks(R)), dim3(MR_THREADS), 0, st, masks, boxes, R, M, H, W,
                     threshold, windows);
  GLASS_CHECK_LAUNCH("glass_roi_mask_windows");
  return GLASS_OK;
}

extern "C" int glass_roi_mask_rings_count(const float* masks, const float* boxes, int R, int M, int H, int W, float threshold,
                                          const int* windows, void* workspace, int64_t workspace_bytes, int* ring_off, int* status,
                                          glass_stream_t stream) {
  if (int rc = roi_args_ok("glass_roi_mask_rings_count", R, M, H, W, threshold)) return rc;
  if (R == 0) return GLASS_OK;
  GLASS_CHECK_ARG(masks && boxes && windows && workspace && ring_off && status, "glass_roi_mask_rings_count: null pointer");
  return rings_count("glass_roi_mask_rings_count", R, H, W, windows, workspace, workspace_bytes, ring_off, status, (hipStream_t)stream,
                     [&](dim3 g, hipStream_t st, const long long* pix_off, int* labels, int* cnt, unsigned long long*) {
                       hipLaunchKernelGGL(mr_roi_label_init_kernel, g, dim3(MR_THREADS), 0, st, masks, boxes, R, M, H, W, threshold,
                                          windows, pix_off, labels, cnt, status);
                     });
}
