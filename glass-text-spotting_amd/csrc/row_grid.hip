// Text lines aligned into rows, cells, tables and columns (include/glass_hip_feature_grid.h states the contract;
// glass_amd/postprocess/row_grid.py:row_grid_host is the same statement in numpy float64).
//
// Three launches, each ordered after the one before by the stream:
//   rg_prep_kernel   one workgroup of 1024 threads per image, thread = line: the page frame by a fixed 1024-slot tree sum and
//                    every valid line's intervals [ulo, uhi], [vlo, vhi], mu, mv and h - the formulas of lo_prep_kernel
//                    (line_order.hip), restated here and kept by line index: nothing below needs an order of the lines.
//   rg_rel_kernel    one wavefront per (image, 64-row block): lane = column line, a loop over the block's rows, and the ballots
//                    of rowmate(a, b) and of over(a, b) && near(a, b) (the two conditions of colmate that need no row) are the
//                    64-bit row words rowm[a][b / 64] and colc[a][b / 64] in the workspace.
//   rg_grid_kernel   one workgroup of 1024 threads per image, thread = line.  The thread keeps its own two rows of words in
//                    registers (a 1024 x 1024 bit relation is 128 KB: no workgroup could stage it in LDS, and nobody but the
//                    line itself reads its row); LDS holds one label, key and number per line, 49 KB in all.  Rows are the
//                    components of rowmate; a line is multi-cell iff its rowmate row is not empty; the colc words then lose
//                    the lines of single-line rows and of the line's own row and are the colmate words; columns are their
//                    components and tables the components of both sets of words together.  Components: minimum-label
//                    propagation with hooking and a pointer jump per round (rg_components), stopped by the first round
//                    without a change and bounded by L rounds; a shuffled path of 1024 lines takes 10 rounds, where the
//                    propagation alone takes 796.  Then every number as a count of smaller keys, the boxes as minima and
//                    maxima in index order by the component's smallest line, and the outputs.
// All arithmetic is float64 without fused multiply-add, the only atomics are integer minima in LDS, and nothing here waits for
// the host.
// Rows beyond the count are never read; a neighbour's index is a bit position below L by the mask put on every word, and
// every other index is computed here, not read.
#include "common.h"
#include "glass_hip_feature_grid.h"

#pragma clang fp contract(off)

constexpr int RG_KMAX = GLASS_ROW_GRID_MAX_K;
constexpr int RG_THREADS = 1024;
constexpr int RG_ROW_WORDS = RG_KMAX / 64;
static_assert(RG_THREADS == RG_KMAX && RG_KMAX % 64 == 0, "one thread per line; the tree sum covers RG_KMAX slots");

typedef unsigned long long rg_u64;

struct RGParams { double row_ov, row_hr, col_ov, gap; };

// the workspace of one image, in 8-byte words: rowm | colc | seven double arrays by line, P_U | valid int [K]
struct RGLayout {
  long rowm, colc, dbl, ints, total;
  int W;
};
enum { RG_ULO = 0, RG_UHI, RG_VLO, RG_VHI, RG_MU, RG_MV, RG_H, RG_DBL_ARRAYS };   // double [K] each, then P_U.x, P_U.y

__host__ __device__ inline RGLayout rg_layout(int K) {
  RGLayout y;
  y.W = (K + 63) / 64;
  const long KW = (long)K * y.W;
  y.rowm = 0;
  y.colc = KW;
  y.dbl = 2 * KW;
  y.ints = y.dbl + (long)RG_DBL_ARRAYS * K + 2;
  y.total = (y.ints + ((long)K + 1) / 2 + 1) / 2 * 2;                             // a 16-byte multiple
  return y;
}

struct RGLine { double cx, cy, w, h, ux, uy; bool valid; };

// one line from its row: widened exactly, valid iff all five finite and w, h > 0; u = (cos t, -sin t), t = a pi / 180
__device__ inline RGLine rg_load(const float* b) {
  const float f0 = b[0], f1 = b[1], f2 = b[2], f3 = b[3], f4 = b[4];
  RGLine q;
  q.valid = isfinite(f0) && isfinite(f1) && isfinite(f2) && isfinite(f3) && isfinite(f4) && f2 > 0.f && f3 > 0.f;
  q.cx = (double)f0; q.cy = (double)f1; q.w = (double)f2; q.h = (double)f3;
  q.ux = 1.0; q.uy = 0.0;
  if (q.valid) {
    const double t = (double)f4 * 3.14159265358979323846 / 180.0;
    q.ux = cos(t); q.uy = -sin(t);
  }
  return q;
}

// the bits of word k that stand for lines below x
__device__ __forceinline__ rg_u64 rg_below(int x, int k) {
  const int d = x - 64 * k;
  return d <= 0 ? 0ull : (d >= 64 ? ~0ull : ((1ull << d) - 1ull));
}

// ------------------------------------------------------------------------------------------------ frame and intervals
__global__ __launch_bounds__(RG_THREADS) void rg_prep_kernel(const float* __restrict__ boxes, const int* __restrict__ count, int K,
                                                             rg_u64* __restrict__ ws) {
  __shared__ double s_dx[RG_KMAX], s_dy[RG_KMAX], s_sw[RG_KMAX];           // the tree sums
  const int img = blockIdx.x, t = threadIdx.x;
  const int n = min(max(count[img], 0), K);
  const RGLayout y = rg_layout(K);
  rg_u64* base = ws + (long)img * y.total;
  double* dbl = reinterpret_cast<double*>(base + y.dbl);
  int* ints = reinterpret_cast<int*>(base + y.ints);

  RGLine q{0., 0., 0., 0., 1., 0., false};
  if (t < n) q = rg_load(boxes + ((long)img * K + t) * 5);
  s_dx[t] = q.valid ? q.w * q.ux : 0.0;
  s_dy[t] = q.valid ? q.w * q.uy : 0.0;
  s_sw[t] = q.valid ? q.w : 0.0;
  __syncthreads();
  for (int stride = RG_KMAX / 2; stride > 0; stride >>= 1) {
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
  if (t < n) {
    dbl[RG_ULO * K + t] = ulo; dbl[RG_UHI * K + t] = uhi; dbl[RG_VLO * K + t] = vlo; dbl[RG_VHI * K + t] = vhi;
    dbl[RG_MU * K + t] = mu; dbl[RG_MV * K + t] = mv; dbl[RG_H * K + t] = q.valid ? q.h : 0.0;
    ints[t] = q.valid ? 1 : 0;
  }
  if (t == 0) { dbl[RG_DBL_ARRAYS * K] = PUx; dbl[RG_DBL_ARRAYS * K + 1] = PUy; }
}

// ------------------------------------------------------------------------------------------------ the two pairwise relations
__global__ __launch_bounds__(64) void rg_rel_kernel(const int* __restrict__ count, int K, RGParams p, rg_u64* __restrict__ ws) {
  __shared__ double s_ulo[64], s_uhi[64], s_vlo[64], s_vhi[64], s_h[64];  // the block's rows
  __shared__ int s_valid[64];
  const int img = blockIdx.y, rb = blockIdx.x, lane = threadIdx.x;
  const int L = min(max(count[img], 0), K);
  if (rb * 64 >= L) return;
  const RGLayout y = rg_layout(K);
  rg_u64* base = ws + (long)img * y.total;
  const double* dbl = reinterpret_cast<const double*>(base + y.dbl);
  const int* ints = reinterpret_cast<const int*>(base + y.ints);
  const int rows = min(64, L - rb * 64), nb = (L + 63) / 64, W = y.W;
  {
    const int i = rb * 64 + lane;
    const bool in = lane < rows;
    s_ulo[lane] = in ? dbl[RG_ULO * K + i] : 0.0; s_uhi[lane] = in ? dbl[RG_UHI * K + i] : 0.0;
    s_vlo[lane] = in ? dbl[RG_VLO * K + i] : 0.0; s_vhi[lane] = in ? dbl[RG_VHI * K + i] : 0.0;
    s_h[lane] = in ? dbl[RG_H * K + i] : 0.0;
    s_valid[lane] = in ? (ints[i] != 0 ? 1 : 0) : 0;
  }
  __syncthreads();
  rg_u64* rowm = base + y.rowm;
  rg_u64* colc = base + y.colc;
  for (int jb = 0; jb < nb; ++jb) {
    const int j = jb * 64 + lane;
    const bool jin = j < L;
    const bool jv = jin && ints[j] != 0;
    const double uloj = jin ? dbl[RG_ULO * K + j] : 0.0, uhij = jin ? dbl[RG_UHI * K + j] : 0.0;
    const double vloj = jin ? dbl[RG_VLO * K + j] : 0.0, vhij = jin ? dbl[RG_VHI * K + j] : 0.0;
    const double hj = jin ? dbl[RG_H * K + j] : 0.0;
    const double ulenj = uhij - uloj, vlenj = vhij - vloj;
    rg_u64 mine_r = 0ull, mine_c = 0ull;
    for (int ii = 0; ii < rows; ++ii) {
      const int i = rb * 64 + ii;                                   // (wavefront-uniform: the reads of line i are broadcasts)
      const double uloi = s_ulo[ii], uhii = s_uhi[ii], vloi = s_vlo[ii], vhii = s_vhi[ii], hi = s_h[ii];
      const bool pair = jv && s_valid[ii] != 0 && i != j;
      const double ovl = fmin(uhii, uhij) - fmax(uloi, uloj);
      const double hmin = fmin(hi, hj), hmax = fmax(hi, hj);
      const bool rm = pair && ovl <= 0.0 && fmin(vhii, vhij) - fmax(vloi, vloj) >= p.row_ov * fmin(vhii - vloi, vlenj) &&
                      hmin >= p.row_hr * hmax;
      const bool cm = pair && ovl > p.col_ov * fmin(uhii - uloi, ulenj) && fmax(vloi, vloj) - fmin(vhii, vhij) <= p.gap * hmax;
      const rg_u64 mr = __ballot(rm), mc = __ballot(cm);
      if (lane == ii) { mine_r = mr; mine_c = mc; }
    }
    if (lane < rows) {
      rowm[(long)(rb * 64 + lane) * W + jb] = mine_r;
      colc[(long)(rb * 64 + lane) * W + jb] = mine_c;
    }
  }
}

// ------------------------------------------------------------------------------------------------ components, numbers, outputs
// exclusive prefix sum of v over the workgroup's threads; `total` is the sum.  s_w: 16 ints of LDS, free again on return.
__device__ __forceinline__ int rg_scan(int v, int* s_w, int& total) {
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
  for (int w = 0; w < RG_THREADS / 64; ++w) {
    const int x = s_w[w];
    before += w < wave ? x : 0;
    all += x;
  }
  __syncthreads();
  total = all;
  return before + inc - v;
}

// The smallest line of thread t's component under the symmetric relation whose row t is w[0 .. nb).  s_a and s_b hold the same
// labels when a round starts.  A line reads the smallest label m among its own and its neighbours' from s_a and gives it, by
// integer minimum in s_b, to itself and to the line its own label names (hooking: a whole tree of labels moves at once); then,
// reading s_b only, it takes the label of its label (the jump), and both arrays get the result.  A round reads what the round
// before left and an integer minimum does not depend on the order of its operands, so every round is deterministic.  Labels
// only fall, stay inside the component and are never above those of the plain propagation, which walks a path of L lines in
// L - 1 rounds; a round that lowers no label has left every line's label no larger than its neighbours', which only the
// component's smallest line everywhere satisfies.  The loop ends with that round, or after L rounds.  Called by all threads.
__device__ __forceinline__ int rg_components(const rg_u64 (&w)[RG_ROW_WORDS], int nb, int L, int* s_a, int* s_b) {
  const int t = threadIdx.x;
  int lab = t;
  s_a[t] = t; s_b[t] = t;
  __syncthreads();
  for (int round = 0; round < L; ++round) {
    int m = lab;
#pragma unroll
    for (int k = 0; k < RG_ROW_WORDS; ++k) {
      if (k < nb) {
        rg_u64 word = w[k];
        while (word) {
          const int b = __ffsll((long long)word) - 1;
          word &= word - 1ull;
          m = min(m, s_a[k * 64 + b]);
        }
      }
    }
    if (m < lab) { atomicMin(&s_b[t], m); atomicMin(&s_b[lab], m); }  // (lab <= t: a label is a line of this workgroup)
    __syncthreads();
    const int jump = s_b[s_b[t]];
    __syncthreads();                                                 // (every read of s_b is behind this barrier)
    s_a[t] = jump; s_b[t] = jump;
    const bool changed = jump != lab;
    lab = jump;
    if (!__syncthreads_or(changed ? 1 : 0)) break;
  }
  return lab;
}

struct RGExtent { double umin, umax, vmin, vmax; };

__device__ __forceinline__ void rg_store_box(float* bb, const RGExtent& e, double PUx, double PUy) {
  const double PVx = -PUy, PVy = PUx;
  const double cu = (e.umin + e.umax) / 2, cv = (e.vmin + e.vmax) / 2;
  bb[0] = (float)(cu * PUx + cv * PVx); bb[1] = (float)(cu * PUy + cv * PVy);
  bb[2] = (float)(e.umax - e.umin); bb[3] = (float)(e.vmax - e.vmin);
  bb[4] = (float)(atan2(-PUy, PUx) * 180.0 / 3.14159265358979323846);
}

__global__ __launch_bounds__(RG_THREADS) void rg_grid_kernel(const float* __restrict__ boxes, const int* __restrict__ count,
                                                             const int* __restrict__ line_start, int K,
                                                             const rg_u64* __restrict__ ws, int* __restrict__ row_id,
                                                             int* __restrict__ row_pos, int* __restrict__ table_id,
                                                             int* __restrict__ col_id, int* __restrict__ row_order,
                                                             int* __restrict__ row_start, float* __restrict__ row_boxes,
                                                             int* __restrict__ row_count, float* __restrict__ table_boxes,
                                                             int* __restrict__ table_rows, int* __restrict__ table_cols,
                                                             int* __restrict__ table_count, int* __restrict__ row_first) {
  __shared__ double s_x[RG_KMAX], s_y[RG_KMAX];           // mv, then the row's smallest mv, then the column's smallest ulo | mu, then ulo
  __shared__ int s_la[RG_KMAX], s_lb[RG_KMAX];            // the labels of rg_components; later the table's smallest row | the position's line
  __shared__ int s_row[RG_KMAX], s_col[RG_KMAX], s_tab[RG_KMAX], s_rowid[RG_KMAX], s_pos[RG_KMAX];
  __shared__ unsigned char s_flag[RG_KMAX];               // 1 a valid line, 2 a line of a multi-cell row
  __shared__ rg_u64 s_multi[RG_ROW_WORDS];
  __shared__ int s_scan[RG_THREADS / 64];
  const int img = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int L = min(max(count[img], 0), K);
  const RGLayout y = rg_layout(K);
  const rg_u64* base = ws + (long)img * y.total;
  const double* dbl = reinterpret_cast<const double*>(base + y.dbl);
  const int* ints = reinterpret_cast<const int*>(base + y.ints);
  const int W = y.W, nb = (L + 63) / 64;
  const bool in = t < L;
  const bool valid = in && ints[t] != 0;
  const long o = (long)img * K;
  double PUx = 1.0, PUy = 0.0;
  if (L > 0) { PUx = dbl[RG_DBL_ARRAYS * K]; PUy = dbl[RG_DBL_ARRAYS * K + 1]; }

  // ---- the line's two rows of words, its keys
  rg_u64 R[RG_ROW_WORDS], C[RG_ROW_WORDS];
  bool multi = false;
#pragma unroll
  for (int k = 0; k < RG_ROW_WORDS; ++k) {
    const bool take = valid && k < nb;
    R[k] = take ? (base + y.rowm)[(long)t * W + k] & rg_below(L, k) : 0ull;
    C[k] = take ? (base + y.colc)[(long)t * W + k] & rg_below(L, k) : 0ull;
    multi = multi || R[k] != 0ull;
  }
  const double mu = valid ? dbl[RG_MU * K + t] : 0.0, mv = valid ? dbl[RG_MV * K + t] : 0.0;
  const double ulo = valid ? dbl[RG_ULO * K + t] : 0.0;
  s_x[t] = mv; s_y[t] = mu;
  s_flag[t] = (valid ? 1 : 0) | (multi ? 2 : 0);
  {
    const rg_u64 m = __ballot(multi);
    if (lane == 0) s_multi[wave] = m;
  }

  // ---- rows
  const int rowlab = rg_components(R, nb, L, s_la, s_lb);            // (its barriers publish the arrays above)
  s_row[t] = rowlab;
  __syncthreads();

  // ---- columns: colmate = over and near, both in multi-cell rows, in different rows; tables: both relations together
#pragma unroll
  for (int k = 0; k < RG_ROW_WORDS; ++k) {
    if (k < nb) {
      rg_u64 word = multi ? C[k] & s_multi[k] : 0ull, keep = word;
      while (word) {
        const int b = __ffsll((long long)word) - 1;
        word &= word - 1ull;
        if (s_row[k * 64 + b] == rowlab) keep &= ~(1ull << b);
      }
      C[k] = keep;
    } else {
      C[k] = 0ull;
    }
  }
  const int collab = rg_components(C, nb, L, s_la, s_lb);
#pragma unroll
  for (int k = 0; k < RG_ROW_WORDS; ++k) C[k] |= R[k];
  const int tablab = rg_components(C, nb, L, s_la, s_lb);
  s_col[t] = collab; s_tab[t] = tablab;

  // ---- per row: the smallest mv, the cell's number, and (by the row's smallest line) the extent
  const bool row_root = valid && rowlab == t;
  double rmin = mv;
  int pos = 0;
  RGExtent re{0., 0., 0., 0.};
  if (valid) {
    if (row_root) re = RGExtent{ulo, dbl[RG_UHI * K + t], dbl[RG_VLO * K + t], dbl[RG_VHI * K + t]};
    for (int j = 0; j < L; ++j) {
      if ((s_flag[j] & 1) && s_row[j] == rowlab) {
        const double mvj = s_x[j], muj = s_y[j];
        rmin = fmin(rmin, mvj);
        pos += (muj < mu || (muj == mu && j < t)) ? 1 : 0;
        if (row_root) {
          re.umin = fmin(re.umin, dbl[RG_ULO * K + j]); re.umax = fmax(re.umax, dbl[RG_UHI * K + j]);
          re.vmin = fmin(re.vmin, dbl[RG_VLO * K + j]); re.vmax = fmax(re.vmax, dbl[RG_VHI * K + j]);
        }
      }
    }
  }
  const int V = __syncthreads_count(valid ? 1 : 0);                  // (every read of mv and mu is behind this barrier)
  s_x[t] = rmin; s_y[t] = ulo; s_pos[t] = pos;
  const int n_valid_rows = __syncthreads_count(row_root ? 1 : 0);

  // ---- the row's number: the rows with a smaller key; an invalid line after all of them, in index order
  int rid = 0;
  if (valid) {
    for (int j = 0; j < L; ++j) {
      if ((s_flag[j] & 1) && s_row[j] == j) {
        const double rj = s_x[j];
        rid += (rj < rmin || (rj == rmin && j < rowlab)) ? 1 : 0;
      }
    }
  } else if (in) {
    rid = n_valid_rows;
    for (int j = 0; j < t; ++j) rid += (s_flag[j] & 1) ? 0 : 1;
  }
  s_rowid[t] = rid;
  __syncthreads();
  const int n_rows = n_valid_rows + (L - V);

  // ---- the line's place in row_order: the lines of the rows ahead, then the cells ahead
  int offset = 0;
  if (in)
    for (int j = 0; j < L; ++j) offset += s_rowid[j] < rid ? 1 : 0;
  const int place = offset + pos;
  if (in) s_lb[place] = t;                                           // (a permutation of 0 .. L - 1)

  // ---- per column: the smallest ulo; per table: the smallest row, the rows, the columns, the extent
  const bool tab_root = multi && tablab == t;
  double cmin = ulo;
  int tmin = rid, trows = 0, tcols = 0;
  RGExtent te{0., 0., 0., 0.};
  if (multi) {
    if (tab_root) te = RGExtent{ulo, dbl[RG_UHI * K + t], dbl[RG_VLO * K + t], dbl[RG_VHI * K + t]};
    for (int j = 0; j < L; ++j) {
      if (s_flag[j] & 2) {
        if (s_tab[j] == tablab) {
          tmin = min(tmin, s_rowid[j]);
          trows += s_pos[j] == 0 ? 1 : 0;
          tcols += s_col[j] == j ? 1 : 0;
          if (tab_root) {
            te.umin = fmin(te.umin, dbl[RG_ULO * K + j]); te.umax = fmax(te.umax, dbl[RG_UHI * K + j]);
            te.vmin = fmin(te.vmin, dbl[RG_VLO * K + j]); te.vmax = fmax(te.vmax, dbl[RG_VHI * K + j]);
          }
        }
        if (s_col[j] == collab) cmin = fmin(cmin, s_y[j]);
      }
    }
  }
  __syncthreads();                                                   // (every read of the rows' smallest mv is behind this barrier)
  s_x[t] = cmin; s_la[t] = tmin;
  const int n_tables = __syncthreads_count(tab_root ? 1 : 0);

  // ---- the table's number and the column's number inside it
  int tid = -1, cid = -1;
  if (multi) {
    tid = 0; cid = 0;
    for (int j = 0; j < L; ++j) {
      if (s_flag[j] & 2) {
        if (s_tab[j] == j) tid += s_la[j] < tmin ? 1 : 0;
        if (s_col[j] == j && s_tab[j] == tablab) {
          const double cj = s_x[j];
          cid += (cj < cmin || (cj == cmin && j < collab)) ? 1 : 0;
        }
      }
    }
  }

  // ---- words ahead of the line, by place in row_order
  if (line_start != nullptr) {
    int size = 0, line = 0;
    if (in) {
      const int* ls = line_start + (long)img * (K + 1);
      line = s_lb[t];
      const int a = ls[line], b = ls[line + 1];
      size = (a >= 0 && a <= b && b <= K) ? b - a : 0;
    }
    int all = 0;
    const int ahead = rg_scan(size, s_scan, all);
    if (in) row_first[o + line] = ahead;
    else if (t < K) row_first[o + t] = -1;
  }

  // ---- the outputs: by line, by place, by row, by table
  if (in) {
    row_id[o + t] = rid; row_pos[o + t] = pos; table_id[o + t] = tid; col_id[o + t] = cid;
    row_order[o + t] = s_lb[t];
    if (row_root) {
      row_start[(long)img * (K + 1) + rid] = offset;
      rg_store_box(row_boxes + (o + rid) * 5, re, PUx, PUy);
    } else if (!valid) {
      row_start[(long)img * (K + 1) + rid] = offset;
      const unsigned* src = reinterpret_cast<const unsigned*>(boxes + (o + t) * 5);
      unsigned* dst = reinterpret_cast<unsigned*>(row_boxes + (o + rid) * 5);
      for (int e = 0; e < 5; ++e) dst[e] = src[e];
    }
    if (tab_root) {
      rg_store_box(table_boxes + (o + tid) * 5, te, PUx, PUy);
      table_rows[o + tid] = trows; table_cols[o + tid] = tcols;
    }
  } else if (t < K) {
    row_id[o + t] = -1; row_pos[o + t] = -1; table_id[o + t] = -1; col_id[o + t] = -1; row_order[o + t] = -1;
  }
  if (t >= n_rows && t < K)
    for (int e = 0; e < 5; ++e) row_boxes[(o + t) * 5 + e] = 0.f;
  if (t >= n_tables && t < K) {
    for (int e = 0; e < 5; ++e) table_boxes[(o + t) * 5 + e] = 0.f;
    table_rows[o + t] = 0; table_cols[o + t] = 0;
  }
  for (int e = n_rows + t; e <= K; e += RG_THREADS) row_start[(long)img * (K + 1) + e] = L;
  if (t == 0) { row_count[img] = n_rows; table_count[img] = n_tables; }
}

extern "C" int64_t glass_row_grid_workspace_bytes(int N, int K) {
  if (N < 0 || K < 0 || K > RG_KMAX) return -1;
  return K == 0 ? 0 : (int64_t)N * rg_layout(K).total * 8;           // (without lines the one launch touches no workspace)
}

extern "C" int glass_row_grid(const float* line_boxes, const int* line_count, const int* line_start, int N, int K,
                              const double* params4_host, int* row_id, int* row_pos, int* table_id, int* col_id, int* row_order,
                              int* row_start, float* row_boxes, int* row_count, float* table_boxes, int* table_rows,
                              int* table_cols, int* table_count, int* row_first, void* workspace, int64_t workspace_bytes,
                              glass_stream_t stream) {
  GLASS_CHECK_ARG(N >= 0, "glass_row_grid: N=%d", N);
  GLASS_CHECK_ARG(K >= 0 && K <= RG_KMAX, "glass_row_grid: K=%d (max %d)", K, RG_KMAX);
  GLASS_CHECK_ARG(params4_host, "glass_row_grid: null parameters");
  RGParams p{params4_host[0], params4_host[1], params4_host[2], params4_host[3]};
  GLASS_CHECK_ARG(p.row_ov > 0 && p.row_ov <= 1, "glass_row_grid: row_min_overlap=%g (0 < . <= 1)", p.row_ov);
  GLASS_CHECK_ARG(p.row_hr >= 0 && p.row_hr <= 1, "glass_row_grid: row_min_height_ratio=%g (0..1)", p.row_hr);
  GLASS_CHECK_ARG(p.col_ov >= 0 && p.col_ov < 1, "glass_row_grid: column_min_overlap=%g (0 <= . < 1)", p.col_ov);
  GLASS_CHECK_ARG(p.gap >= 0 && p.gap <= 1.7e308, "glass_row_grid: table_max_row_gap=%g (finite, >= 0)", p.gap);
  GLASS_CHECK_ARG(K == 0 || (line_start == nullptr) == (row_first == nullptr), "glass_row_grid: line_start and row_first go together");
  if (N == 0) return GLASS_OK;
  GLASS_CHECK_ARG(line_count && row_start && row_count && table_count, "glass_row_grid: null pointer");
  GLASS_CHECK_ARG(K == 0 || (line_boxes && row_id && row_pos && table_id && col_id && row_order && row_boxes && table_boxes &&
                             table_rows && table_cols), "glass_row_grid: null pointer");
  const int64_t need = glass_row_grid_workspace_bytes(N, K);
  GLASS_CHECK_ARG(need == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need),
                  "glass_row_grid: workspace of %lld bytes (16-byte aligned), needs %lld", (long long)workspace_bytes,
                  (long long)need);
  rg_u64* ws = static_cast<rg_u64*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (K > 0) {
    const int W = rg_layout(K).W;
    hipLaunchKernelGGL(rg_prep_kernel, dim3(N), dim3(RG_THREADS), 0, st, line_boxes, line_count, K, ws);
    GLASS_CHECK_LAUNCH("glass_row_grid (prep)");
    hipLaunchKernelGGL(rg_rel_kernel, dim3(W, N), dim3(64), 0, st, line_count, K, p, ws);
    GLASS_CHECK_LAUNCH("glass_row_grid (relations)");
  }
  hipLaunchKernelGGL(rg_grid_kernel, dim3(N), dim3(RG_THREADS), 0, st, line_boxes, line_count, line_start, K,
                     static_cast<const rg_u64*>(ws), row_id, row_pos, table_id, col_id, row_order, row_start, row_boxes, row_count,
                     table_boxes, table_rows, table_cols, table_count, row_first);
  GLASS_CHECK_LAUNCH("glass_row_grid (grid)");
  return GLASS_OK;
}
