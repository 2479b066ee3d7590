// Pose graph: the solve (include/voxgraph_amd.h).  Levenberg-Marquardt over the 4-DoF node poses: registration constraints
// through a vgx_reg_batch, relative-pose edges on the host in f64, and the reduced normal equations assembled, damped,
// factorised (right-looking Cholesky, 64-wide panels: dense, or over the stored 64 x 64 tiles alone) and solved on the
// device in f64.  Every number follows the order contract of the header: built with -ffp-contract=off, one rounded
// multiply and one rounded subtract at a time.
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <set>

#include "vgx_internal.h"
#include "vgx_tile_pattern.h"

using namespace vgx;

namespace {

constexpr int kPanel = 64;          // panel width = tile size of the factorisation
constexpr int kMaxFreeNodes = 4096;
constexpr int kMaxDenseN = 4 * kMaxFreeNodes;
constexpr int kEdgeTermDoubles = 56;  // per edge on the device: g_a[4] g_b[4] aa[16] bb[16] ab[16]

// ---------------------------------------------------------------------------
// assembly: gather through index lists, fixed order, no atomics
// ---------------------------------------------------------------------------
struct BlockRecord {
  int32_t bi, bj;        // block row / column in the reduced matrix
  int32_t first, count;  // its items
};
// item = (offset << 2) | (source << 1) | transpose; source 0: the fused buffer, 1: the edge terms
__global__ void pg_assemble_blocks_kernel(const BlockRecord* __restrict__ blocks, int n_blocks, const int32_t* __restrict__ items,
                                          const double* __restrict__ fused, const double* __restrict__ edge, double* __restrict__ H,
                                          int nf) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_blocks * 16) return;
  const BlockRecord B = blocks[t >> 4];
  const int e = t & 15, r = e >> 2, c = e & 3;
  double acc = 0.0;
  for (int k = 0; k < B.count; ++k) {
    const int32_t it = items[B.first + k];
    const double* src = (it & 2) ? edge : fused;
    acc = acc + src[(size_t)(it >> 2) + ((it & 1) ? c * 4 + r : e)];
  }
  H[(size_t)(4 * B.bi + r) * nf + 4 * B.bj + c] = acc;
}
// per free node: records {first, count}; item = (offset << 1) | source
__global__ void pg_assemble_gradient_kernel(const int32_t* __restrict__ first, const int32_t* __restrict__ items,
                                            const double* __restrict__ fused, const double* __restrict__ edge, double* __restrict__ g,
                                            int n_free_nodes) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_free_nodes * 4) return;
  const int node = t >> 2, k = t & 3;
  double acc = 0.0;
  for (int i = first[node]; i < first[node + 1]; ++i) {
    const int32_t it = items[i];
    const double* src = (it & 1) ? edge : fused;
    acc = acc + src[(size_t)(it >> 1) + k];
  }
  g[t] = acc;
}
// element [0] of every constraint's 45-block
__global__ void pg_gather_cost_kernel(const double* __restrict__ normal, int n, double* __restrict__ cost) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) cost[c] = normal[(size_t)c * kNormalSize];
}
// A = H on the diagonal plus clip(H_ii, 1e-6, 1e32) / radius (A holds a copy of H already)
__global__ void pg_damp_kernel(const double* __restrict__ H, double* __restrict__ A, int nf, double radius) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf) return;
  const double h = H[(size_t)i * nf + i];
  const double d2 = h < 1e-6 ? 1e-6 : (h > 1e32 ? 1e32 : h);  // (a NaN stays a NaN, as numpy's clip leaves it)
  A[(size_t)i * nf + i] = h + d2 / radius;
}

// ---------------------------------------------------------------------------
// Cholesky, right-looking, 64-wide panels (lower triangle of row-major A, in place)
// ---------------------------------------------------------------------------
// 1. the diagonal tile, one workgroup, in LDS
__global__ __launch_bounds__(256) void pg_chol_diag_kernel(double* __restrict__ A, int n, int k0, int w, int* __restrict__ flag) {
  if (*flag) return;
  __shared__ double T[kPanel * (kPanel + 1)];
  const int tid = threadIdx.x;
  for (int e = tid; e < kPanel * kPanel; e += 256) {
    const int i = e >> 6, j = e & 63;
    T[i * (kPanel + 1) + j] = (i < w && j <= i) ? A[(size_t)(k0 + i) * n + k0 + j] : 0.0;
  }
  __syncthreads();
  bool bad = false;
  for (int k = 0; k < w; ++k) {
    const double akk = T[k * (kPanel + 1) + k];
    if (!(akk > 0.0) || isinf(akk)) bad = true;
    const double lkk = sqrt(akk);
    __syncthreads();
    if (tid == 0) T[k * (kPanel + 1) + k] = lkk;
    if (tid > k && tid < w) T[tid * (kPanel + 1) + k] = T[tid * (kPanel + 1) + k] / lkk;
    __syncthreads();
    for (int e = tid; e < kPanel * kPanel; e += 256) {
      const int i = e >> 6, j = e & 63;
      if (j > k && j <= i && i < w)
        T[i * (kPanel + 1) + j] = T[i * (kPanel + 1) + j] - T[i * (kPanel + 1) + k] * T[j * (kPanel + 1) + k];
    }
    __syncthreads();
  }
  for (int e = tid; e < kPanel * kPanel; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (i < w && j <= i) A[(size_t)(k0 + i) * n + k0 + j] = T[i * (kPanel + 1) + j];
  }
  if (bad && tid == 0) *flag = 1;
}

// ---------------------------------------------------------------------------
// The arithmetic the dense and the tile-sparse factorisation share, written once: both compile to the instruction
// streams they had with these lines written out in each kernel.  The substitutions' shared steps (the triangle fill,
// the one-wavefront triangle solve, the panel phase of the many-column solve) stay written out per kernel: as
// helpers they cost time on the device (profiles/pose_graph_shared_time.txt).
// ---------------------------------------------------------------------------
// one row of the panel below a factored tile against that tile's packed triangle Lt: (c, j) at c (c + 1) / 2 + j
__device__ __forceinline__ void chol_panel_row_solve(double* row, const double* Lt, int w) {
  for (int j = 0; j < w; ++j) {
    const double x = row[j] / Lt[j * (j + 1) / 2 + j];
    row[j] = x;
    for (int c = j + 1; c < w; ++c) row[c] = row[c] - x * Lt[c * (c + 1) / 2 + j];
  }
}
// acc -= a b^T for one staged column, product by product: a = pa[0 .. 3], b = pb[0 .. 3] (in LDS, 16-byte aligned).
// One rounded multiply and one rounded subtract at a time, never a sum of products.  The loop over the columns stays
// with the caller: its order is the caller's (ascending, or descending in a backward pass), and so is its unrolling.
__device__ __forceinline__ void rank_update_4x4(double (&acc)[4][4], const double* pa, const double* pb) {
  const double2 a01 = *reinterpret_cast<const double2*>(pa), a23 = *reinterpret_cast<const double2*>(pa + 2);
  const double2 b01 = *reinterpret_cast<const double2*>(pb), b23 = *reinterpret_cast<const double2*>(pb + 2);
  const double av[4] = {a01.x, a01.y, a23.x, a23.y};
  const double bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] - av[a] * bv[b];
}

// 2. the panel below it: 64 rows per workgroup, one row per lane, against the factored tile
__global__ __launch_bounds__(64) void pg_chol_panel_kernel(double* __restrict__ A, int n, int k0, int w, const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ double Lt[kPanel * (kPanel + 1) / 2];  // packed lower triangle: (c, j) at c (c + 1) / 2 + j
  __shared__ double R[kPanel * (kPanel + 1)];
  const int t = threadIdx.x;
  const int row0 = k0 + w + blockIdx.x * kPanel;
  for (int r = 0; r < w; ++r)
    if (t <= r) Lt[r * (r + 1) / 2 + t] = A[(size_t)(k0 + r) * n + k0 + t];
  for (int r = 0; r < kPanel; ++r)
    R[r * (kPanel + 1) + t] = (row0 + r < n && t < w) ? A[(size_t)(row0 + r) * n + k0 + t] : 0.0;
  __syncthreads();
  if (row0 + t < n) chol_panel_row_solve(R + t * (kPanel + 1), Lt, w);
  __syncthreads();
  for (int r = 0; r < kPanel; ++r)
    if (row0 + r < n && t < w) A[(size_t)(row0 + r) * n + k0 + t] = R[r * (kPanel + 1) + t];
}

// 3. the trailing tiles on or below the diagonal: a 64 x 64 tile per workgroup, a 4 x 4 micro-tile per thread; the
// accumulators START from the stored a_ij and subtract product by product in ascending k (never a sum of products)
constexpr int kChunk = 32;            // panel columns staged per pass
constexpr int kStride = kPanel + 2;   // LDS row stride of a staged chunk, [k][row]: 16-byte aligned rows
__global__ __launch_bounds__(256) void pg_chol_trailing_kernel(double* __restrict__ A, int n, int k0, int w, int tile0,
                                                              const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ alignas(16) double PI[kChunk * kStride];
  __shared__ alignas(16) double PJ[kChunk * kStride];
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > t) --I;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  const int J = t - I * (I + 1) / 2;
  const int i0 = (tile0 + I) * kPanel, j0 = (tile0 + J) * kPanel;
  const int ty = tid >> 4, tx = tid & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int row = i0 + ty * 4 + a, col = j0 + tx * 4 + b;
      acc[a][b] = (row < n && col <= row) ? A[(size_t)row * n + col] : 0.0;
    }
  for (int kc = 0; kc < w; kc += kChunk) {
    __syncthreads();
    {
      const int k = tid & (kChunk - 1);
      for (int r = tid / kChunk; r < kPanel; r += 256 / kChunk) {
        const bool in_k = kc + k < w;
        PI[k * kStride + r] = (in_k && i0 + r < n) ? A[(size_t)(i0 + r) * n + k0 + kc + k] : 0.0;
        PJ[k * kStride + r] = (in_k && j0 + r < n) ? A[(size_t)(j0 + r) * n + k0 + kc + k] : 0.0;
      }
    }
    __syncthreads();
    const int kn = min(kChunk, w - kc);
    for (int k = 0; k < kn; ++k) rank_update_4x4(acc, &PI[k * kStride + ty * 4], &PJ[k * kStride + tx * 4]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int row = i0 + ty * 4 + a, col = j0 + tx * 4 + b;
      if (row < n && col <= row) A[(size_t)row * n + col] = acc[a][b];
    }
}

// ---------------------------------------------------------------------------
// substitutions: one workgroup, column-oriented, panel by panel (b in place)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void pg_forward_kernel(const double* __restrict__ L, int n, double* __restrict__ b) {
  __shared__ double Lt[kPanel * (kPanel + 1)];
  __shared__ double yb[kPanel];
  const int tid = threadIdx.x;
  for (int k0 = 0; k0 < n; k0 += kPanel) {
    const int w = min(kPanel, n - k0);
    for (int e = tid; e < kPanel * kPanel; e += 1024) {
      const int i = e >> 6, j = e & 63;
      Lt[i * (kPanel + 1) + j] = (i < w && j <= i) ? L[(size_t)(k0 + i) * n + k0 + j] : 1.0;
    }
    __syncthreads();
    if (tid < 64) {  // the panel's own triangle: one wavefront, the running value of row `tid` in a register
      double y = tid < w ? b[k0 + tid] : 0.0;
      for (int j = 0; j < w; ++j) {
        if (tid == j) y = y / Lt[j * (kPanel + 1) + j];
        const double yj = __shfl(y, j);
        if (tid > j) y = y - Lt[tid * (kPanel + 1) + j] * yj;
      }
      yb[tid] = y;
      if (tid < w) b[k0 + tid] = y;
    }
    __syncthreads();
    for (int i = k0 + w + tid; i < n; i += 1024) {
      double acc = b[i];
      const double* row = L + (size_t)i * n + k0;
      for (int k = 0; k < w; ++k) acc = acc - row[k] * yb[k];
      b[i] = acc;
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(1024) void pg_backward_kernel(const double* __restrict__ L, int n, double* __restrict__ b) {
  __shared__ double Lt[kPanel * (kPanel + 1)];
  __shared__ double xb[kPanel];
  const int tid = threadIdx.x;
  for (int k0 = ((n - 1) / kPanel) * kPanel; k0 >= 0; k0 -= kPanel) {
    const int w = min(kPanel, n - k0);
    for (int e = tid; e < kPanel * kPanel; e += 1024) {
      const int i = e >> 6, j = e & 63;
      Lt[i * (kPanel + 1) + j] = (i < w && j <= i) ? L[(size_t)(k0 + i) * n + k0 + j] : 1.0;
    }
    __syncthreads();
    if (tid < 64) {
      double y = tid < w ? b[k0 + tid] : 0.0;
      for (int j = w - 1; j >= 0; --j) {
        if (tid == j) y = y / Lt[j * (kPanel + 1) + j];
        const double xj = __shfl(y, j);
        if (tid < j) y = y - Lt[j * (kPanel + 1) + tid] * xj;
      }
      xb[tid] = y;
      if (tid < w) b[k0 + tid] = y;
    }
    __syncthreads();
    for (int i = tid; i < k0; i += 1024) {
      double acc = b[i];
      for (int k = w - 1; k >= 0; --k) acc = acc - L[(size_t)(k0 + k) * n + i] * xb[k];
      b[i] = acc;
    }
    __syncthreads();
  }
}
// ---------------------------------------------------------------------------
// substitutions on many right-hand sides: X [n][m] row-major, in place; a workgroup owns kSolveCols columns and walks
// the panels alone, so the two passes are one launch each and no workgroup waits for another
// ---------------------------------------------------------------------------
constexpr int kSolveCols = 32;                         // columns of X per workgroup
constexpr int kSolveColGroups = kSolveCols / 4;        // 4 x 4 micro-tiles: column groups ...
constexpr int kSolveRowGroups = 256 / kSolveColGroups; // ... and row groups of one pass of the row update
constexpr int kSolveRows = 4 * kSolveRowGroups;        // rows of X updated per pass
constexpr int kSolveK = 4096 / kSolveRows;             // columns of L staged per pass: 32 KB of LDS
constexpr int kSolveStride = kSolveRows + 2;           // LDS row stride of the staged columns, [k][row]
constexpr int kSolveYStride = kSolveCols + 2;          // ... and of the panel's solved rows, [k][column]
constexpr int kSolveColsPerWave = kSolveCols / 4;
constexpr int kSolveStage = kSolveK * kSolveStride > kPanel * (kPanel + 1) ? kSolveK * kSolveStride : kPanel * (kPanel + 1);
static_assert(kSolveCols % 16 == 0 && kSolveCols <= 64 && kSolveK <= kPanel && kPanel % kSolveK == 0, "the shape of pg_solve_many_kernel");

// row j of a wavefront's columns, column q in lane q: their divisions by l_jj are then ONE division for the wavefront
// (the same operands per column, so the same bits) and not one per column
__device__ __forceinline__ double pivot_row(const double (&y)[kSolveColsPerWave], int j, int lane) {
  double d = 0.0;
#pragma unroll
  for (int q = 0; q < kSolveColsPerWave; ++q) {
    const double v = __shfl(y[q], j);
    if (lane == q) d = v;
  }
  return d;
}

// chunk_rows (nullable): per workgroup {the first row of its columns that is not zero, the lowest row wanted of them}.
// Every element's history is that of pg_forward_kernel / pg_backward_kernel: the triangle in one wavefront per column
// (kSolveColsPerWave columns interleaved), the other rows from accumulators that START at the stored value and subtract
// product by product, k ascending (forward) or descending (backward).
template <bool kBackward>
__global__ __launch_bounds__(256) void pg_solve_many_kernel(const double* __restrict__ L, int n, double* __restrict__ X, int m,
                                                           const int32_t* __restrict__ chunk_rows, const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ alignas(16) double S[kSolveStage];  // the panel's triangle, then the staged columns of L
  __shared__ alignas(16) double Y[kPanel * kSolveYStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid % kSolveColGroups, ty = tid / kSolveColGroups;
  const int c0 = blockIdx.x * kSolveCols;
  const int n_panels = (n + kPanel - 1) / kPanel;
  // Unit right-hand sides.  Forward: the panels above a column's 1 are skipped -- there b_i = 0 and every y_k so far is
  // +0.0, and with a factor that passed the pivot check (finite: an inf or NaN below the diagonal reaches a later pivot)
  // 0.0 - l * 0.0 = +0.0 and +0.0 / l_ii = +0.0, which is what X holds already.  Backward: the pass stops after the
  // panel of the lowest row wanted -- the rows above it take no part in the rows below.  No delivered bit changes.
  const int p_first = (!kBackward && chunk_rows) ? chunk_rows[2 * blockIdx.x] / kPanel : 0;
  const int p_last = (kBackward && chunk_rows) ? chunk_rows[2 * blockIdx.x + 1] / kPanel : 0;
  for (int p = kBackward ? n_panels - 1 : p_first; kBackward ? p >= p_last : p < n_panels; p += kBackward ? -1 : 1) {
    const int k0 = p * kPanel, w = min(kPanel, n - k0);
    __syncthreads();
    for (int e = tid; e < kPanel * kPanel; e += 256) {
      const int i = e >> 6, j = e & 63;
      S[i * (kPanel + 1) + j] = (i < w && j <= i) ? L[(size_t)(k0 + i) * n + k0 + j] : 1.0;
    }
    for (int e = tid; e < kPanel * kSolveCols; e += 256) {
      const int r = e / kSolveCols, c = e % kSolveCols;
      Y[r * kSolveYStride + c] = (r < w && c0 + c < m) ? X[(size_t)(k0 + r) * m + c0 + c] : 0.0;
    }
    __syncthreads();
    {  // the panel's own triangle: row `lane` of this wavefront's columns in registers
      double y[kSolveColsPerWave];
#pragma unroll
      for (int q = 0; q < kSolveColsPerWave; ++q) y[q] = Y[lane * kSolveYStride + wave * kSolveColsPerWave + q];
      if (!kBackward) {
        for (int j = 0; j < w; ++j) {
          const double ljj = S[j * (kPanel + 1) + j], lij = lane > j ? S[lane * (kPanel + 1) + j] : 0.0;
          const double d = pivot_row(y, j, lane) / ljj;
#pragma unroll
          for (int q = 0; q < kSolveColsPerWave; ++q) {
            const double yj = __shfl(d, q);
            if (lane == j) y[q] = yj;
            if (lane > j) y[q] = y[q] - lij * yj;
          }
        }
      } else {
        for (int j = w - 1; j >= 0; --j) {
          const double ljj = S[j * (kPanel + 1) + j], lji = lane < j ? S[j * (kPanel + 1) + lane] : 0.0;
          const double d = pivot_row(y, j, lane) / ljj;
#pragma unroll
          for (int q = 0; q < kSolveColsPerWave; ++q) {
            const double xj = __shfl(d, q);
            if (lane == j) y[q] = xj;
            if (lane < j) y[q] = y[q] - lji * xj;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kSolveColsPerWave; ++q) Y[lane * kSolveYStride + wave * kSolveColsPerWave + q] = y[q];
    }
    __syncthreads();
    for (int e = tid; e < kPanel * kSolveCols; e += 256) {
      const int r = e / kSolveCols, c = e % kSolveCols;
      if (r < w && c0 + c < m) X[(size_t)(k0 + r) * m + c0 + c] = Y[r * kSolveYStride + c];
    }
    // the other rows: below the panel (forward), above it down to the last panel's first row (backward)
    const int row_begin = kBackward ? p_last * kPanel : k0 + w, row_end = kBackward ? k0 : n;
    for (int i0 = row_begin; i0 < row_end; i0 += kSolveRows) {
      double acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int row = i0 + ty * 4 + a, col = c0 + tx * 4 + b;
          acc[a][b] = (row < row_end && col < m) ? X[(size_t)row * m + col] : 0.0;
        }
      const int n_passes = (w + kSolveK - 1) / kSolveK;
      for (int s = 0; s < n_passes; ++s) {
        const int kc = (kBackward ? n_passes - 1 - s : s) * kSolveK;
        __syncthreads();
        if (!kBackward) {  // S[k][r] = l(i0 + r, k0 + kc + k): a row of L per kSolveK threads
          const int k = tid % kSolveK;
          for (int r = tid / kSolveK; r < kSolveRows; r += 256 / kSolveK)
            S[k * kSolveStride + r] = (kc + k < w && i0 + r < row_end) ? L[(size_t)(i0 + r) * n + k0 + kc + k] : 0.0;
        } else {           // S[k][r] = l(k0 + kc + k, i0 + r): a row of L per kSolveRows threads
          const int r = tid % kSolveRows;
          for (int k = tid / kSolveRows; k < kSolveK; k += 256 / kSolveRows)
            S[k * kSolveStride + r] = (kc + k < w && i0 + r < row_end) ? L[(size_t)(k0 + kc + k) * n + i0 + r] : 0.0;
        }
        __syncthreads();
        const int kn = min(kSolveK, w - kc);
        for (int kk = 0; kk < kn; ++kk) {
          const int k = kBackward ? kn - 1 - kk : kk;
          rank_update_4x4(acc, &S[k * kSolveStride + ty * 4], &Y[(kc + k) * kSolveYStride + tx * 4]);
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int row = i0 + ty * 4 + a, col = c0 + tx * 4 + b;
          if (row < row_end && col < m) X[(size_t)row * m + col] = acc[a][b];
        }
    }
  }
}
// X [n][m] = the columns unit_row[c] of the identity
__global__ void pg_unit_columns_kernel(double* __restrict__ X, int n, int m, const int32_t* __restrict__ unit_row) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * m) return;
  const int i = (int)(t / m), c = (int)(t % m);
  X[t] = unit_row[c] == i ? 1.0 : 0.0;
}
// out [n_pairs][16] = the 4x4 block of X at rows block[2p] .. + 3, columns block[2p + 1] .. + 3; zeros where either is
// negative (a constant node).  out[16 n_pairs] = the factorisation's flag, so that one copy brings both.
__global__ void pg_gather_blocks_kernel(const double* __restrict__ X, int m, const int32_t* __restrict__ block, int n_pairs,
                                        const int* __restrict__ flag, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) out[(size_t)n_pairs * 16] = (double)*flag;
  if (t >= n_pairs * 16) return;
  const int p = t >> 4, r = (t >> 2) & 3, c = t & 3;
  const int32_t row = block[2 * p], col = block[2 * p + 1];
  out[t] = (row < 0 || col < 0) ? 0.0 : X[(size_t)(row + r) * m + col + c];
}

// step = -z, Hs = H step (per row, ascending columns, from 0.0); out = [step nf][Hs nf]
__global__ void pg_negate_kernel(const double* __restrict__ z, double* __restrict__ out, int nf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nf) out[i] = -z[i];
}
__global__ __launch_bounds__(64) void pg_matvec_kernel(const double* __restrict__ H, double* __restrict__ out, int nf) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nf) return;
  const double* row = H + (size_t)r * nf;
  double acc = 0.0;
  for (int c = 0; c < nf; ++c) acc = acc + row[c] * out[c];
  out[nf + r] = acc;
}

// queues the factorisation of the n x n matrix A on the context's stream; *d_flag becomes 1 at a bad pivot (ctx->mu held)
int queue_cholesky(vgx_ctx ctx, double* A, int n, int* d_flag) {
  VGX_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  const int n_tiles = (n + kPanel - 1) / kPanel;
  for (int k0 = 0; k0 < n; k0 += kPanel) {
    const int w = std::min(kPanel, n - k0);
    hipLaunchKernelGGL(pg_chol_diag_kernel, dim3(1), dim3(256), 0, ctx->stream, A, n, k0, w, d_flag);
    const int below = n - k0 - w;
    if (below > 0) {
      hipLaunchKernelGGL(pg_chol_panel_kernel, dim3((below + kPanel - 1) / kPanel), dim3(64), 0, ctx->stream, A, n, k0, w, d_flag);
      const int tile0 = k0 / kPanel + 1, m = n_tiles - tile0;
      hipLaunchKernelGGL(pg_chol_trailing_kernel, dim3(m * (m + 1) / 2), dim3(256), 0, ctx->stream, A, n, k0, w, tile0, d_flag);
    }
  }
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}
// ... and of the two substitutions on the right-hand side in d_x (in place)
int queue_substitutions(vgx_ctx ctx, const double* L, int n, double* d_x) {
  hipLaunchKernelGGL(pg_forward_kernel, dim3(1), dim3(1024), 0, ctx->stream, L, n, d_x);
  hipLaunchKernelGGL(pg_backward_kernel, dim3(1), dim3(1024), 0, ctx->stream, L, n, d_x);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

// ... and of the two substitutions on the m columns of d_X [n][m] (in place): two launches.  d_chunk_rows: nullable,
// [ceil(m / kSolveCols)][2], see pg_solve_many_kernel
int queue_solve_many(vgx_ctx ctx, const double* L, int n, double* d_X, int m, const int32_t* d_chunk_rows, const int* d_flag) {
  const dim3 grid((m + kSolveCols - 1) / kSolveCols);
  hipLaunchKernelGGL(pg_solve_many_kernel<false>, grid, dim3(256), 0, ctx->stream, L, n, d_X, m, d_chunk_rows, d_flag);
  hipLaunchKernelGGL(pg_solve_many_kernel<true>, grid, dim3(256), 0, ctx->stream, L, n, d_X, m, d_chunk_rows, d_flag);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

// ---------------------------------------------------------------------------
// the tile-sparse solver: H and A / L as arrays of 64 x 64 tiles (row-major inside a tile), the structure of
// vgx_tile_pattern.h.  A tile that is structurally zero in L is not stored, read or updated; every stored element has
// the history of the dense kernels above less the products with an exact zero factor.
// ---------------------------------------------------------------------------
constexpr int kTileDoubles = kPanel * kPanel;
static_assert(kPanel == kTile, "one tile per panel");

// the 4x4 block of record b lies in tile block_tile[b] of H; bi / bj are positions in the order in use
__global__ void pg_assemble_blocks_tiled_kernel(const BlockRecord* __restrict__ blocks, const int32_t* __restrict__ block_tile, int n_blocks,
                                                const int32_t* __restrict__ items, const double* __restrict__ fused,
                                                const double* __restrict__ edge, double* __restrict__ Ht) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_blocks * 16) return;
  const BlockRecord B = blocks[t >> 4];
  const int e = t & 15, r = e >> 2, c = e & 3;
  double acc = 0.0;
  for (int k = 0; k < B.count; ++k) {
    const int32_t it = items[B.first + k];
    const double* src = (it & 2) ? edge : fused;
    acc = acc + src[(size_t)(it >> 2) + ((it & 1) ? c * 4 + r : e)];
  }
  Ht[(size_t)block_tile[t >> 4] * kTileDoubles + (4 * (B.bi % kNodesPerTile) + r) * kPanel + 4 * (B.bj % kNodesPerTile) + c] = acc;
}
// A's tiles start as copies of H's; a tile of pure fill starts at +0.0
__global__ __launch_bounds__(256) void pg_tiles_from_h_kernel(const double* __restrict__ Ht, double* __restrict__ At,
                                                              const int32_t* __restrict__ l_from_h) {
  const int32_t src = l_from_h[blockIdx.x];
  double2* dst = reinterpret_cast<double2*>(At + (size_t)blockIdx.x * kTileDoubles);
  const double2* from = reinterpret_cast<const double2*>(Ht + (size_t)(src < 0 ? 0 : src) * kTileDoubles);
  for (int e = threadIdx.x; e < kTileDoubles / 2; e += 256) dst[e] = src < 0 ? make_double2(0.0, 0.0) : from[e];
}
__global__ void pg_damp_tiled_kernel(const double* __restrict__ Ht, double* __restrict__ At, const int32_t* __restrict__ h_diag,
                                     const int32_t* __restrict__ col_first, int nf, double radius) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf) return;
  const int K = i / kPanel, e = (i % kPanel) * (kPanel + 1);
  const double h = Ht[(size_t)h_diag[K] * kTileDoubles + e];
  const double d2 = h < 1e-6 ? 1e-6 : (h > 1e32 ? 1e32 : h);
  At[(size_t)col_first[K] * kTileDoubles + e] = h + d2 / radius;
}

// 1. the diagonal tile: pg_chol_diag_kernel on the tile's pointer (n = 64, k0 = 0)
// 2. the stored tiles of column K below it, one per workgroup: tiles first + 1 + blockIdx.x of the list
__global__ __launch_bounds__(64) void pg_chol_panel_tiled_kernel(double* __restrict__ At, int first, const int32_t* __restrict__ l_row,
                                                                 int n, const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ double Lt[kPanel * (kPanel + 1) / 2];
  __shared__ double R[kPanel * (kPanel + 1)];
  const int t = threadIdx.x;
  const int tile = first + 1 + blockIdx.x;
  const double* D = At + (size_t)first * kTileDoubles;
  double* T = At + (size_t)tile * kTileDoubles;
  const int rows = min(kPanel, n - l_row[tile] * kPanel);
  for (int r = 0; r < kPanel; ++r)
    if (t <= r) Lt[r * (r + 1) / 2 + t] = D[r * kPanel + t];
  for (int r = 0; r < kPanel; ++r) R[r * (kPanel + 1) + t] = r < rows ? T[r * kPanel + t] : 0.0;
  __syncthreads();
  if (t < rows) chol_panel_row_solve(R + t * (kPanel + 1), Lt, kPanel);
  __syncthreads();
  for (int r = 0; r < rows; ++r) T[r * kPanel + t] = R[r * (kPanel + 1) + t];
}
// 3. the update triples of panel K, one per workgroup: pg_chol_trailing_kernel's micro-tile, accumulators that start
// from the stored value, the subtract inside the k loop
__global__ __launch_bounds__(256) void pg_chol_trailing_tiled_kernel(double* __restrict__ At, const TileTriple* __restrict__ triples,
                                                                    const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ alignas(16) double PI[kChunk * kStride];
  __shared__ alignas(16) double PJ[kChunk * kStride];
  const int tid = threadIdx.x;
  const TileTriple tr = triples[blockIdx.x];
  double* T = At + (size_t)tr.target * kTileDoubles;
  const double* SI = At + (size_t)tr.source_i * kTileDoubles;
  const double* SJ = At + (size_t)tr.source_j * kTileDoubles;
  const int rows_i = tr.rows & 255, rows_j = (tr.rows >> 8) & 255;
  const bool diagonal = (tr.rows >> 16) != 0;
  const int ty = tid >> 4, tx = tid & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int row = ty * 4 + a, col = tx * 4 + b;
      acc[a][b] = (row < rows_i && (!diagonal || col <= row)) ? T[row * kPanel + col] : 0.0;
    }
  for (int kc = 0; kc < kPanel; kc += kChunk) {
    __syncthreads();
    {
      const int k = tid & (kChunk - 1);
      for (int r = tid / kChunk; r < kPanel; r += 256 / kChunk) {
        PI[k * kStride + r] = r < rows_i ? SI[r * kPanel + kc + k] : 0.0;
        PJ[k * kStride + r] = r < rows_j ? SJ[r * kPanel + kc + k] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll  // (whole, as the compiler chose for these lines written out; through the call it would stop at four)
    for (int k = 0; k < kChunk; ++k) rank_update_4x4(acc, &PI[k * kStride + ty * 4], &PJ[k * kStride + tx * 4]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int row = ty * 4 + a, col = tx * 4 + b;
      if (row < rows_i && (!diagonal || col <= row)) T[row * kPanel + col] = acc[a][b];
    }
}

// the substitutions of pg_forward_kernel / pg_backward_kernel: after a panel's triangle the rows of the column's
// stored tiles alone (forward), the columns of the row's stored tiles alone (backward); 16 tiles per pass, a row or a
// column per thread, the same k order
__global__ __launch_bounds__(1024) void pg_forward_tiled_kernel(const double* __restrict__ Lt_, const int32_t* __restrict__ col_first,
                                                               const int32_t* __restrict__ l_row, int n, double* __restrict__ b) {
  __shared__ double Lt[kPanel * (kPanel + 1)];
  __shared__ double yb[kPanel];
  const int tid = threadIdx.x;
  const int n_panels = (n + kPanel - 1) / kPanel;
  for (int K = 0; K < n_panels; ++K) {
    const int k0 = K * kPanel, w = min(kPanel, n - k0);
    const int first = col_first[K], n_below = col_first[K + 1] - first - 1;
    const double* D = Lt_ + (size_t)first * kTileDoubles;
    for (int e = tid; e < kPanel * kPanel; e += 1024) {
      const int i = e >> 6, j = e & 63;
      Lt[i * (kPanel + 1) + j] = (i < w && j <= i) ? D[i * kPanel + j] : 1.0;
    }
    __syncthreads();
    if (tid < 64) {
      double y = tid < w ? b[k0 + tid] : 0.0;
      for (int j = 0; j < w; ++j) {
        if (tid == j) y = y / Lt[j * (kPanel + 1) + j];
        const double yj = __shfl(y, j);
        if (tid > j) y = y - Lt[tid * (kPanel + 1) + j] * yj;
      }
      yb[tid] = y;
      if (tid < w) b[k0 + tid] = y;
    }
    __syncthreads();
    for (int q = tid >> 6; q < n_below; q += 16) {
      const int tile = first + 1 + q, r = tid & 63, i = l_row[tile] * kPanel + r;
      if (i < n) {
        double acc = b[i];
        const double* row = Lt_ + (size_t)tile * kTileDoubles + r * kPanel;
        for (int k = 0; k < w; ++k) acc = acc - row[k] * yb[k];
        b[i] = acc;
      }
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(1024) void pg_backward_tiled_kernel(const double* __restrict__ Lt_, const int32_t* __restrict__ col_first,
                                                                const int32_t* __restrict__ row_first, const int32_t* __restrict__ row_tile,
                                                                const int32_t* __restrict__ row_col, int n, double* __restrict__ b) {
  __shared__ double Lt[kPanel * (kPanel + 1)];
  __shared__ double xb[kPanel];
  const int tid = threadIdx.x;
  for (int K = (n - 1) / kPanel; K >= 0; --K) {
    const int k0 = K * kPanel, w = min(kPanel, n - k0);
    const double* D = Lt_ + (size_t)col_first[K] * kTileDoubles;
    for (int e = tid; e < kPanel * kPanel; e += 1024) {
      const int i = e >> 6, j = e & 63;
      Lt[i * (kPanel + 1) + j] = (i < w && j <= i) ? D[i * kPanel + j] : 1.0;
    }
    __syncthreads();
    if (tid < 64) {
      double y = tid < w ? b[k0 + tid] : 0.0;
      for (int j = w - 1; j >= 0; --j) {
        if (tid == j) y = y / Lt[j * (kPanel + 1) + j];
        const double xj = __shfl(y, j);
        if (tid < j) y = y - Lt[j * (kPanel + 1) + tid] * xj;
      }
      xb[tid] = y;
      if (tid < w) b[k0 + tid] = y;
    }
    __syncthreads();
    for (int q = row_first[K] + (tid >> 6); q < row_first[K + 1]; q += 16) {
      const int c = tid & 63, i = row_col[q] * kPanel + c;  // (a column left of the diagonal tile: i < n)
      const double* T = Lt_ + (size_t)row_tile[q] * kTileDoubles;
      double acc = b[i];
      for (int k = w - 1; k >= 0; --k) acc = acc - T[k * kPanel + c] * xb[k];
      b[i] = acc;
    }
    __syncthreads();
  }
}
// ---------------------------------------------------------------------------
// the tiled substitutions on many right-hand sides: pg_solve_many_kernel over the tile lists.  X [n][m] row-major, in
// place; a workgroup owns kSolveCols columns and walks the panels alone.  After a panel's triangle only the stored tiles
// of the panel's column (forward) or row (backward) are updated -- two tiles per pass with the 4 x 4 micro-tile, a last
// single tile with a 2 x 4 one, so that all 256 threads have rows either way.
// ---------------------------------------------------------------------------
static_assert(kSolveRows == 2 * kPanel && kSolveK * 2 == kPanel, "pg_solve_many_tiled_kernel takes two tiles per pass, half a tile's k range at a time");

// One pass of the row update: kTiles tiles (32 kTiles rows of X per row group of threads, R = 2 kTiles rows per thread).
// T[h]: the tile, i0[h]: the first row of X it updates, rows[h]: how many.  Forward: x_(i0 + r) -= T[r][k] y_k, k ascending;
// backward: x_(i0 + r) -= T[k][r] x_k, k descending from w - 1.  The accumulators START at the stored value.
template <bool kBackward, int kTiles>
__device__ __forceinline__ void solve_many_tiles_pass(const double* const (&T)[2], const int (&i0)[2], const int (&rows)[2], int w,
                                                      double* __restrict__ X, int m, int c0, double* __restrict__ S,
                                                      const double* __restrict__ Y, int tid) {
  constexpr int R = 2 * kTiles;
  const int tx = tid % kSolveColGroups, ty = tid / kSolveColGroups;
  const int lr0 = ty * R, h = lr0 >> 6, rt0 = lr0 & (kPanel - 1);  // (R | 64: a thread's rows lie in one tile)
  double acc[R][4];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = c0 + tx * 4 + b;
      acc[a][b] = (rt0 + a < rows[h] && col < m) ? X[(size_t)(i0[h] + rt0 + a) * m + col] : 0.0;
    }
  const int n_passes = (w + kSolveK - 1) / kSolveK;
  for (int s = 0; s < n_passes; ++s) {
    const int kc = (kBackward ? n_passes - 1 - s : s) * kSolveK;
    __syncthreads();
    if (!kBackward) {  // S[k][lr] = T[lr / 64][lr % 64][kc + k]: a tile row per kSolveK threads
      const int k = tid % kSolveK;
      for (int lr = tid / kSolveK; lr < kPanel * kTiles; lr += 256 / kSolveK) {
        const int hh = lr >> 6, rt = lr & (kPanel - 1);
        S[k * kSolveStride + lr] = (kc + k < w && rt < rows[hh]) ? T[hh][rt * kPanel + kc + k] : 0.0;
      }
    } else {           // S[k][lr] = T[lr / 64][kc + k][lr % 64]: a tile row per 64 threads
      const int lr = tid % (kPanel * kTiles), hh = lr >> 6, rt = lr & (kPanel - 1);
      for (int k = tid / (kPanel * kTiles); k < kSolveK; k += 256 / (kPanel * kTiles))
        S[k * kSolveStride + lr] = (kc + k < w && rt < rows[hh]) ? T[hh][(kc + k) * kPanel + rt] : 0.0;
    }
    __syncthreads();
    const int kn = min(kSolveK, w - kc);
    for (int kk = 0; kk < kn; ++kk) {
      const int k = kBackward ? kn - 1 - kk : kk;
      double av[R];
#pragma unroll
      for (int a = 0; a < R; a += 2) {
        const double2 v = *reinterpret_cast<const double2*>(&S[k * kSolveStride + lr0 + a]);
        av[a] = v.x, av[a + 1] = v.y;
      }
      const double2 b01 = *reinterpret_cast<const double2*>(&Y[(kc + k) * kSolveYStride + tx * 4]);
      const double2 b23 = *reinterpret_cast<const double2*>(&Y[(kc + k) * kSolveYStride + tx * 4 + 2]);
      const double bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] - av[a] * bv[b];
    }
  }
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = c0 + tx * 4 + b;
      if (rt0 + a < rows[h] && col < m) X[(size_t)(i0[h] + rt0 + a) * m + col] = acc[a][b];
    }
}

// chunk_rows (nullable): as for pg_solve_many_kernel, the rows being positions in the order in use.  The two skips keep
// that kernel's argument: above the panel of a unit column's 1 every y is +0.0 (a finite factor), and the rows above
// the panel of the lowest row wanted take no part in the rows below -- so a tile whose column lies left of that panel is
// not updated in the backward pass.  Every delivered element has the history of pg_forward_tiled_kernel /
// pg_backward_tiled_kernel on its column.
template <bool kBackward>
__global__ __launch_bounds__(256) void pg_solve_many_tiled_kernel(const double* __restrict__ Lt_, const int32_t* __restrict__ col_first,
                                                                 const int32_t* __restrict__ l_row, const int32_t* __restrict__ row_first,
                                                                 const int32_t* __restrict__ row_tile, const int32_t* __restrict__ row_col,
                                                                 int n, double* __restrict__ X, int m,
                                                                 const int32_t* __restrict__ chunk_rows, const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ alignas(16) double S[kSolveStage];  // the panel's triangle, then the staged halves of one or two tiles
  __shared__ alignas(16) double Y[kPanel * kSolveYStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * kSolveCols;
  const int n_panels = (n + kPanel - 1) / kPanel;
  const int p_first = (!kBackward && chunk_rows) ? chunk_rows[2 * blockIdx.x] / kPanel : 0;
  const int p_last = (kBackward && chunk_rows) ? chunk_rows[2 * blockIdx.x + 1] / kPanel : 0;
  for (int p = kBackward ? n_panels - 1 : p_first; kBackward ? p >= p_last : p < n_panels; p += kBackward ? -1 : 1) {
    const int k0 = p * kPanel, w = min(kPanel, n - k0);
    const int first = col_first[p];
    const double* D = Lt_ + (size_t)first * kTileDoubles;
    __syncthreads();
    for (int e = tid; e < kPanel * kPanel; e += 256) {
      const int i = e >> 6, j = e & 63;
      S[i * (kPanel + 1) + j] = (i < w && j <= i) ? D[i * kPanel + j] : 1.0;
    }
    for (int e = tid; e < kPanel * kSolveCols; e += 256) {
      const int r = e / kSolveCols, c = e % kSolveCols;
      Y[r * kSolveYStride + c] = (r < w && c0 + c < m) ? X[(size_t)(k0 + r) * m + c0 + c] : 0.0;
    }
    __syncthreads();
    {  // the panel's own triangle: row `lane` of this wavefront's columns in registers
      double y[kSolveColsPerWave];
#pragma unroll
      for (int q = 0; q < kSolveColsPerWave; ++q) y[q] = Y[lane * kSolveYStride + wave * kSolveColsPerWave + q];
      if (!kBackward) {
        for (int j = 0; j < w; ++j) {
          const double ljj = S[j * (kPanel + 1) + j], lij = lane > j ? S[lane * (kPanel + 1) + j] : 0.0;
          const double d = pivot_row(y, j, lane) / ljj;
#pragma unroll
          for (int q = 0; q < kSolveColsPerWave; ++q) {
            const double yj = __shfl(d, q);
            if (lane == j) y[q] = yj;
            if (lane > j) y[q] = y[q] - lij * yj;
          }
        }
      } else {
        for (int j = w - 1; j >= 0; --j) {
          const double ljj = S[j * (kPanel + 1) + j], lji = lane < j ? S[j * (kPanel + 1) + lane] : 0.0;
          const double d = pivot_row(y, j, lane) / ljj;
#pragma unroll
          for (int q = 0; q < kSolveColsPerWave; ++q) {
            const double xj = __shfl(d, q);
            if (lane == j) y[q] = xj;
            if (lane < j) y[q] = y[q] - lji * xj;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < kSolveColsPerWave; ++q) Y[lane * kSolveYStride + wave * kSolveColsPerWave + q] = y[q];
    }
    __syncthreads();
    for (int e = tid; e < kPanel * kSolveCols; e += 256) {
      const int r = e / kSolveCols, c = e % kSolveCols;
      if (r < w && c0 + c < m) X[(size_t)(k0 + r) * m + c0 + c] = Y[r * kSolveYStride + c];
    }
    // the stored tiles alone: below the diagonal one in the panel's column (forward), left of it in the panel's row
    // down to the last panel's column (backward; the row list ascends by column)
    int q = kBackward ? row_first[p] : first + 1;
    const int q_end = kBackward ? row_first[p + 1] : col_first[p + 1];
    if (kBackward)
      while (q < q_end && row_col[q] < p_last) ++q;
    for (; q < q_end; q += 2) {
      const bool two = q + 1 < q_end;
      const int qa = q, qb = two ? q + 1 : q;
      const double* const T[2] = {Lt_ + (size_t)(kBackward ? row_tile[qa] : qa) * kTileDoubles,
                                  Lt_ + (size_t)(kBackward ? row_tile[qb] : qb) * kTileDoubles};
      const int i0[2] = {(kBackward ? row_col[qa] : l_row[qa]) * kPanel, (kBackward ? row_col[qb] : l_row[qb]) * kPanel};
      const int rows[2] = {min(kPanel, n - i0[0]), min(kPanel, n - i0[1])};
      if (two)
        solve_many_tiles_pass<kBackward, 2>(T, i0, rows, w, X, m, c0, S, Y, tid);
      else
        solve_many_tiles_pass<kBackward, 1>(T, i0, rows, w, X, m, c0, S, Y, tid);
    }
  }
}
// out[16 list[3 t] + e] = the 4x4 block of the slab X [n][m] at rows list[3 t + 1] .. + 3, columns list[3 t + 2] .. + 3
__global__ void pg_gather_slab_blocks_kernel(const double* __restrict__ X, int m, const int32_t* __restrict__ list, int n_list,
                                             double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_list * 16) return;
  const int32_t* rec = list + 3 * (size_t)(t >> 4);
  const int r = (t >> 2) & 3, c = t & 3;
  out[(size_t)rec[0] * 16 + (t & 15)] = X[(size_t)(rec[1] + r) * m + rec[2] + c];
}

// the right-hand side into the order in use: x[4 p + k] = g[4 order[p] + k]
__global__ void pg_permute_kernel(const double* __restrict__ g, const int32_t* __restrict__ order, double* __restrict__ x, int nf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nf) x[i] = g[4 * order[i >> 2] + (i & 3)];
}
// z <- -z (the step in the order in use, for H step), out = the step in ascending node order
__global__ void pg_negate_permuted_kernel(double* __restrict__ z, const int32_t* __restrict__ order, double* __restrict__ out, int nf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf) return;
  const double v = -z[i];
  z[i] = v;
  out[4 * order[i >> 2] + (i & 3)] = v;
}
// H step per row of the order in use: ascending columns over the row's stored tiles, from 0.0; out[nf + the row's
// place in ascending node order]
__global__ __launch_bounds__(64) void pg_matvec_tiled_kernel(const double* __restrict__ Ht, const int32_t* __restrict__ h_row_first,
                                                            const int32_t* __restrict__ h_col, const double* __restrict__ step,
                                                            const int32_t* __restrict__ order, double* __restrict__ out, int nf) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nf) return;
  const int I = r / kPanel;
  double acc = 0.0;
  for (int t = h_row_first[I]; t < h_row_first[I + 1]; ++t) {
    const double* row = Ht + (size_t)t * kTileDoubles + (r % kPanel) * kPanel;
    const int c0 = h_col[t] * kPanel, cn = min(kPanel, nf - c0);
    for (int c = 0; c < cn; ++c) acc = acc + row[c] * step[c0 + c];
  }
  out[nf + 4 * order[r >> 2] + (r & 3)] = acc;
}

// the structure's lists on the device
struct DeviceTiles {
  DeviceArray<int32_t> col_first, l_row, row_first, row_tile, row_col, h_row_first, h_col, h_diag, l_from_h, order;
  DeviceArray<TileTriple> triples;
  size_t bytes = 0;  // of the lists
};
int upload_structure(vgx_ctx ctx, const TileStructure& S, DeviceTiles* d) {
  d->bytes = 0;
  auto up = [&](DeviceBuffer& buf, const void* src, size_t count, size_t size) {
    static const int64_t zero[2] = {0, 0};
    d->bytes += std::max<size_t>(1, count) * size;
    return upload_new(ctx, buf, count ? src : zero, std::max<size_t>(1, count) * size);
  };
  int rc = up(d->col_first, S.col_first.data(), S.col_first.size(), 4);
  if (rc == VGX_OK) rc = up(d->l_row, S.l_row.data(), S.l_row.size(), 4);
  if (rc == VGX_OK) rc = up(d->row_first, S.row_first.data(), S.row_first.size(), 4);
  if (rc == VGX_OK) rc = up(d->row_tile, S.row_tile.data(), S.row_tile.size(), 4);
  if (rc == VGX_OK) rc = up(d->row_col, S.row_col.data(), S.row_col.size(), 4);
  if (rc == VGX_OK) rc = up(d->h_row_first, S.h_row_first.data(), S.h_row_first.size(), 4);
  if (rc == VGX_OK) rc = up(d->h_col, S.h_col.data(), S.h_col.size(), 4);
  if (rc == VGX_OK) rc = up(d->h_diag, S.h_diag.data(), S.h_diag.size(), 4);
  if (rc == VGX_OK) rc = up(d->l_from_h, S.l_from_h.data(), S.l_from_h.size(), 4);
  if (rc == VGX_OK) rc = up(d->order, S.order.data(), S.order.size(), 4);
  if (rc == VGX_OK) rc = up(d->triples, S.triples.data(), S.triples.size(), sizeof(TileTriple));
  return rc;
}
// The tile cap: what the device has free when the structure is made, in 32 KiB tiles (hipMemGetInfo), less `reserve`
// bytes for the graph's other arrays.  n_tiles over it: VGX_ERR_UNSUPPORTED.
int check_tile_cap(vgx_ctx ctx, const char* who, size_t n_tiles, size_t held_bytes, size_t reserve) {
  size_t free_bytes = 0, total = 0;
  VGX_HIP(ctx, hipMemGetInfo(&free_bytes, &total));
  free_bytes += held_bytes;  // (what the handle holds already is given back first)
  const size_t cap = free_bytes > reserve ? (free_bytes - reserve) / (kTileDoubles * sizeof(double)) : 0;
  if (n_tiles > cap || n_tiles >= ((size_t)1 << 31))
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(who) + ": the tiles of H and L number " + std::to_string(n_tiles) +
                                                   "; the tile cap (free device memory / 32 KiB per tile) is " + std::to_string(cap));
  return VGX_OK;
}
// queues the factorisation over the tiles At: 3 launches per panel, 1 for a panel with nothing below its diagonal tile
int queue_cholesky_tiled(vgx_ctx ctx, const TileStructure& S, const DeviceTiles& d, double* At, int n, int* d_flag) {
  VGX_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  for (int K = 0; K < S.n_tile_rows; ++K) {
    const int first = S.col_first[(size_t)K], below = S.col_first[(size_t)K + 1] - first - 1;
    hipLaunchKernelGGL(pg_chol_diag_kernel, dim3(1), dim3(256), 0, ctx->stream, At + (size_t)first * kTileDoubles, kPanel, 0,
                       S.rows_of(K), d_flag);
    if (below > 0) {
      hipLaunchKernelGGL(pg_chol_panel_tiled_kernel, dim3(below), dim3(64), 0, ctx->stream, At, first, d.l_row.get(), n, d_flag);
      const int64_t t0 = S.triple_first[(size_t)K], nt = S.triple_first[(size_t)K + 1] - t0;
      hipLaunchKernelGGL(pg_chol_trailing_tiled_kernel, dim3((unsigned)nt), dim3(256), 0, ctx->stream, At, d.triples.get() + t0, d_flag);
    }
  }
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}
int queue_substitutions_tiled(vgx_ctx ctx, const DeviceTiles& d, const double* Lt, int n, double* d_x) {
  hipLaunchKernelGGL(pg_forward_tiled_kernel, dim3(1), dim3(1024), 0, ctx->stream, Lt, d.col_first.get(), d.l_row.get(), n, d_x);
  hipLaunchKernelGGL(pg_backward_tiled_kernel, dim3(1), dim3(1024), 0, ctx->stream, Lt, d.col_first.get(), d.row_first.get(),
                     d.row_tile.get(), d.row_col.get(), n, d_x);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}
// ... and on the m columns of d_X [n][m] (in place): two launches.  d_chunk_rows: nullable, [ceil(m / kSolveCols)][2]
int queue_solve_many_tiled(vgx_ctx ctx, const DeviceTiles& d, const double* Lt, int n, double* d_X, int m, const int32_t* d_chunk_rows,
                           const int* d_flag) {
  const dim3 grid((m + kSolveCols - 1) / kSolveCols);
  hipLaunchKernelGGL(pg_solve_many_tiled_kernel<false>, grid, dim3(256), 0, ctx->stream, Lt, d.col_first.get(), d.l_row.get(),
                     d.row_first.get(), d.row_tile.get(), d.row_col.get(), n, d_X, m, d_chunk_rows, d_flag);
  hipLaunchKernelGGL(pg_solve_many_tiled_kernel<true>, grid, dim3(256), 0, ctx->stream, Lt, d.col_first.get(), d.l_row.get(),
                     d.row_first.get(), d.row_tile.get(), d.row_col.get(), n, d_X, m, d_chunk_rows, d_flag);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}
// m == 0: one right-hand side through the single-column kernels; m > 0: b and x are [4 n_block_rows][m]
int block_spd_solve(vgx_ctx ctx, const char* who, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj,
                    const double* values, int32_t m, const double* b, double* x, vgx_pose_graph_structure_stats* stats,
                    int32_t* tile_index, double* tile_values);
int launches_per_factorisation(const TileStructure& S) {
  int n = 0;
  for (int K = 0; K < S.n_tile_rows; ++K) n += S.col_first[(size_t)K + 1] - S.col_first[(size_t)K] > 1 ? 3 : 1;
  return n;
}

// ---------------------------------------------------------------------------
// relative-pose edges, host, f64 (relative_pose_cost_function_inl.h:8-70 with analytic Jacobians)
// ---------------------------------------------------------------------------
double normalize_angle(double a) {
  const double two_pi = 2.0 * M_PI;
  return a - two_pi * std::floor((a + M_PI) / two_pi);
}
// cost = r.r; with `terms` also g_a g_b aa bb ab (kEdgeTermDoubles); every sum ascending from 0.0
double edge_terms(const vgx_pose_graph_edge& e, const double* pa, const double* pb, double* terms) {
  const double c = std::cos(pa[3]), s = std::sin(pa[3]);
  const double d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
  const double err[4] = {c * d0 + s * d1 - e.t_obs[0], -s * d0 + c * d1 - e.t_obs[1], d2 - e.t_obs[2],
                         normalize_angle(pb[3] - pa[3] - e.yaw_obs)};
  const double* S = e.sqrt_information;
  double r[4];
  double cost = 0.0;
  for (int i = 0; i < 4; ++i) {
    double acc = 0.0;
    for (int k = 0; k < 4; ++k) acc = acc + S[4 * i + k] * err[k];
    r[i] = acc;
  }
  for (int i = 0; i < 4; ++i) cost = cost + r[i] * r[i];
  if (!terms) return cost;
  double Ja[16] = {0}, Jb[16] = {0};
  Jb[0] = c, Jb[1] = s, Jb[4] = -s, Jb[5] = c, Jb[10] = 1.0, Jb[15] = 1.0;
  for (int i = 0; i < 16; ++i) Ja[i] = -Jb[i];
  Ja[3] = -s * d0 + c * d1;
  Ja[7] = -c * d0 - s * d1;
  double SJa[16], SJb[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double x = 0.0, y = 0.0;
      for (int k = 0; k < 4; ++k) {
        x = x + S[4 * i + k] * Ja[4 * k + j];
        y = y + S[4 * i + k] * Jb[4 * k + j];
      }
      SJa[4 * i + j] = x;
      SJb[4 * i + j] = y;
    }
  double *ga = terms, *gb = terms + 4, *aa = terms + 8, *bb = terms + 24, *ab = terms + 40;
  for (int i = 0; i < 4; ++i) {
    double x = 0.0, y = 0.0;
    for (int k = 0; k < 4; ++k) {
      x = x + SJa[4 * k + i] * r[k];
      y = y + SJb[4 * k + i] * r[k];
    }
    ga[i] = x;
    gb[i] = y;
    for (int j = 0; j < 4; ++j) {
      double p = 0.0, q = 0.0, m = 0.0;
      for (int k = 0; k < 4; ++k) {
        p = p + SJa[4 * k + i] * SJa[4 * k + j];
        q = q + SJb[4 * k + i] * SJb[4 * k + j];
        m = m + SJa[4 * k + i] * SJb[4 * k + j];
      }
      aa[4 * i + j] = p;
      bb[4 * i + j] = q;
      ab[4 * i + j] = m;
    }
  }
  return cost;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct vgx_pose_graph_s {
  vgx_ctx ctx = nullptr;
  int32_t n_nodes = 0;
  std::vector<int32_t> pos;  // node -> index among the free nodes (ascending), or -1: constant
  std::vector<int32_t> free_nodes;
  int nf = 0;                // 4 x free nodes
  vgx_reg_batch batch = nullptr;
  std::vector<vgx_pose_graph_edge> edges;
  std::mutex mu;             // one solve (or setter) at a time
  // the index lists of the assembly, rebuilt when the constraints changed or registration is switched off / on
  bool lists_made = false, lists_with_reg = false, lists_sparse = false;
  int n_blocks = 0;
  // the linear solver; with the tile-sparse one the structure of the lists, its device copy and the tiles of H and A / L
  int32_t solver = VGX_LINEAR_SOLVER_DENSE, ordering = VGX_ORDER_NATURAL;
  std::vector<int32_t> given_order;  // VGX_ORDER_GIVEN: position -> free node
  TileStructure S;
  DeviceTiles tiles;
  DeviceArray<int32_t> d_block_tile;
  DeviceArray<double> d_Ht, d_At;
  size_t sparse_bytes = 0;
  DeviceArray<BlockRecord> d_blocks;
  DeviceArray<int32_t> d_block_items, d_grad_first, d_grad_items;
  // the system
  DeviceArray<double> d_H, d_A, d_g, d_x, d_out, d_fused, d_edge, d_cost;
  DeviceArray<int> d_flag;
  PinnedBuffer h_io;         // doubles: [step nf][H step nf][g nf][edge terms 56 E][costs n] + the flag
  bool system_valid = false;
  std::vector<vgx_pose_graph_iteration> history;
  // vgx_pose_graph_covariance: the solved columns [nf][m <= nf], the index lists, the blocks; grown on demand
  // (vgx_pose_graph_covariance_sparse: d_X is the column slab [nf][S], held within its byte budget)
  DeviceArray<double> d_X, d_cov;
  DeviceArray<int32_t> d_cov_index;
  PinnedBuffer h_cov;        // [blocks 16 n_pairs + the flag, doubles][index lists, int32]
};

namespace {

void release_batch(vgx_pose_graph pg) {
  vgx_reg_batch b = pg->batch;
  if (!b) return;
  pg->batch = nullptr;
  bool destroy = false;
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    destroy = --b->users == 0 && b->destroy_requested;
  }
  if (destroy) (void)vgx_reg_batch_destroy(b);
}

// Index lists in the contract's order.  with_reg: the fused buffer's blocks take part.
int make_lists_unguarded(vgx_pose_graph pg, bool with_reg, bool sparse) {
  vgx_ctx ctx = pg->ctx;
  const int n = pg->n_nodes, nfn = (int)pg->free_nodes.size();
  const vgx_reg_batch b = with_reg ? pg->batch : nullptr;
  const int m = b ? b->n : 0;
  if (vgx_reg_fused_size(n, m) >= (int64_t)1 << 29 || (int64_t)pg->edges.size() * kEdgeTermDoubles >= (int64_t)1 << 29)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_pose_graph_optimize: the constraint list is too long for the 32-bit index lists");
  if (sparse) {  // the structure first: with an ordering the blocks sit at their positions in P H P^T
    std::vector<int32_t> joined;
    auto join = [&](int a, int bb) {
      if (pg->pos[(size_t)a] < 0 || pg->pos[(size_t)bb] < 0) return;
      joined.push_back(pg->pos[(size_t)a]);
      joined.push_back(pg->pos[(size_t)bb]);
    };
    for (int c = 0; c < m; ++c) join(b->node_pair[2 * (size_t)c], b->node_pair[2 * (size_t)c + 1]);
    for (const vgx_pose_graph_edge& e : pg->edges) join(e.a, e.b);
    if (!build_tile_structure(nfn, (int64_t)(joined.size() / 2), joined.data(), pg->ordering, pg->given_order.data(), &pg->S))
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: the ordering is not a permutation of the free nodes");
  }
  std::map<std::pair<int32_t, int32_t>, std::vector<int32_t>> blocks;
  std::vector<std::vector<int32_t>> grad((size_t)nfn);
  auto add = [&](int node_r, int node_c, int64_t offset, int source, int transpose) {
    int32_t r = pg->pos[(size_t)node_r], c = pg->pos[(size_t)node_c];
    if (r < 0 || c < 0) return;
    if (sparse) r = pg->S.position[(size_t)r], c = pg->S.position[(size_t)c];
    blocks[{r, c}].push_back((int32_t)(offset << 2 | source << 1 | transpose));
  };
  if (b) {
    for (int i = 0; i < n; ++i) {  // 1. the fused buffer's diagonal blocks (and its gradient)
      add(i, i, 1 + 4 * (int64_t)n + 16 * (int64_t)i, 0, 0);
      if (pg->pos[(size_t)i] >= 0) grad[(size_t)pg->pos[(size_t)i]].push_back((int32_t)((1 + 4 * (int64_t)i) << 1));
    }
    for (int c = 0; c < m; ++c) {  // 2. the off-diagonal blocks in constraint-list order
      const int a = b->node_pair[2 * (size_t)c], bb = b->node_pair[2 * (size_t)c + 1];
      const int64_t off = 1 + 20 * (int64_t)n + 16 * (int64_t)c;
      add(a, bb, off, 0, 0);
      add(bb, a, off, 0, 1);
    }
  }
  for (size_t e = 0; e < pg->edges.size(); ++e) {  // 3. the edges in list order: aa, bb, ab, ab^T
    const int a = pg->edges[e].a, bb = pg->edges[e].b;
    const int64_t base = (int64_t)e * kEdgeTermDoubles;
    add(a, a, base + 8, 1, 0);
    add(bb, bb, base + 24, 1, 0);
    add(a, bb, base + 40, 1, 0);
    add(bb, a, base + 40, 1, 1);
    if (pg->pos[(size_t)a] >= 0) grad[(size_t)pg->pos[(size_t)a]].push_back((int32_t)(base << 1 | 1));
    if (pg->pos[(size_t)bb] >= 0) grad[(size_t)pg->pos[(size_t)bb]].push_back((int32_t)((base + 4) << 1 | 1));
  }
  std::vector<BlockRecord> records;
  std::vector<int32_t> items, gfirst((size_t)nfn + 1, 0), gitems, block_tile;
  for (const auto& kv : blocks) {
    if (sparse) block_tile.push_back(h_tile(pg->S, kv.first.first / kNodesPerTile, kv.first.second / kNodesPerTile));
    records.push_back({kv.first.first, kv.first.second, (int32_t)items.size(), (int32_t)kv.second.size()});
    items.insert(items.end(), kv.second.begin(), kv.second.end());
  }
  for (int i = 0; i < nfn; ++i) {
    gitems.insert(gitems.end(), grad[(size_t)i].begin(), grad[(size_t)i].end());
    gfirst[(size_t)i + 1] = (int32_t)gitems.size();
  }
  if (items.empty()) items.push_back(0);
  if (gitems.empty()) gitems.push_back(0);
  if (records.empty()) records.push_back({0, 0, 0, 0});
  if (block_tile.empty()) block_tile.push_back(0);
  pg->n_blocks = (int)blocks.size();
  pg->lists_made = false;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int rc = upload_new(ctx, pg->d_blocks, records.data(), records.size() * sizeof(BlockRecord));
  if (rc == VGX_OK) rc = upload_new(ctx, pg->d_block_items, items.data(), items.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, pg->d_grad_first, gfirst.data(), gfirst.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, pg->d_grad_items, gitems.data(), gitems.size() * sizeof(int32_t));
  if (rc != VGX_OK) return rc;
  const size_t nf = (size_t)pg->nf, n_fused = (size_t)vgx_reg_fused_size(n, m), E = pg->edges.size();
  hipError_t e = hipSuccess;
  const size_t n_h = pg->S.h_col.size(), n_l = pg->S.l_row.size(), tile_bytes = kTileDoubles * sizeof(double);
  if (sparse) {
    pg->d_H.release();
    pg->d_A.release();
    pg->d_X.release();
    rc = upload_new(ctx, pg->d_block_tile, block_tile.data(), block_tile.size() * sizeof(int32_t));
    if (rc == VGX_OK) rc = upload_structure(ctx, pg->S, &pg->tiles);
    if (rc == VGX_OK)
      rc = check_tile_cap(ctx, "vgx_pose_graph_optimize", n_h + n_l, pg->d_Ht.bytes + pg->d_At.bytes,
                          (6 * nf + n_fused + E * kEdgeTermDoubles + (size_t)m + 64) * sizeof(double));
    if (rc != VGX_OK) return rc;
    e = pg->d_Ht.reserve(n_h * tile_bytes);
    if (e == hipSuccess) e = pg->d_At.reserve(n_l * tile_bytes);
    pg->sparse_bytes = (n_h + n_l) * tile_bytes + pg->tiles.bytes + block_tile.size() * sizeof(int32_t);
  } else {
    pg->d_Ht.release();
    pg->d_At.release();
    for (DeviceBuffer* buf : {(DeviceBuffer*)&pg->d_H, (DeviceBuffer*)&pg->d_A})
      if (e == hipSuccess) e = buf->reserve(nf * nf * sizeof(double));
  }
  if (e == hipSuccess) e = pg->d_g.reserve(nf * sizeof(double));
  if (e == hipSuccess) e = pg->d_x.reserve(nf * sizeof(double));
  if (e == hipSuccess) e = pg->d_out.reserve(2 * nf * sizeof(double));
  if (e == hipSuccess) e = pg->d_fused.reserve(n_fused * sizeof(double));
  if (e == hipSuccess) e = pg->d_edge.reserve(std::max<size_t>(1, E) * kEdgeTermDoubles * sizeof(double));
  if (e == hipSuccess) e = pg->d_cost.reserve((size_t)std::max(1, m) * sizeof(double));
  if (e == hipSuccess) e = pg->d_flag.reserve(sizeof(int));
  if (e != hipSuccess) return alloc_error(ctx, e, sparse ? "vgx_pose_graph_optimize: allocating the tiles" : "vgx_pose_graph_optimize: allocating the dense system");
  e = pg->h_io.reserve((3 * nf + E * kEdgeTermDoubles + (size_t)m + 2) * sizeof(double));
  if (e != hipSuccess) return alloc_error(ctx, e, "vgx_pose_graph_optimize: allocating the pinned staging");
  // blocks no constraint touches stay zero: the lists never write them
  if (sparse)
    VGX_HIP(ctx, hipMemsetAsync(pg->d_Ht.p, 0, n_h * tile_bytes, ctx->stream));
  else
    VGX_HIP(ctx, hipMemsetAsync(pg->d_H.p, 0, nf * nf * sizeof(double), ctx->stream));
  VGX_HIP(ctx, hipMemsetAsync(pg->d_fused.p, 0, n_fused * sizeof(double), ctx->stream));
  pg->lists_made = true;
  pg->lists_with_reg = with_reg;
  pg->lists_sparse = sparse;
  pg->system_valid = false;
  return VGX_OK;
}

// (the lists and the structure are host containers sized by the caller's graph: out of host memory is a status)
int make_lists(vgx_pose_graph pg, bool with_reg, bool sparse) {
  try {
    return make_lists_unguarded(pg, with_reg, sparse);
  } catch (const std::bad_alloc&) {
    pg->lists_made = false;
    return set_error(pg->ctx, VGX_ERR_NOMEM, "vgx_pose_graph_optimize: out of host memory for the index lists or the tile structure");
  }
}

struct Solve {
  vgx_pose_graph pg;
  bool with_reg;
  double reg_seconds = 0, la_seconds = 0;
  int full_evaluations = 0, cost_evaluations = 0;
  double* h_step() const { return pg->h_io.as<double>(); }
  double* h_Hs() const { return h_step() + pg->nf; }
  double* h_g() const { return h_step() + 2 * (size_t)pg->nf; }
  double* h_edge() const { return h_step() + 3 * (size_t)pg->nf; }
  double* h_costs() const { return h_edge() + pg->edges.size() * kEdgeTermDoubles; }
  int* h_flag() const { return reinterpret_cast<int*>(h_costs() + (with_reg ? pg->batch->n : 0) + 1); }

  double edge_cost(const double* poses, bool terms) const {
    double cost = 0.0;
    for (size_t e = 0; e < pg->edges.size(); ++e) {
      const vgx_pose_graph_edge& E = pg->edges[e];
      cost = cost + edge_terms(E, poses + 4 * (size_t)E.a, poses + 4 * (size_t)E.b, terms ? h_edge() + e * kEdgeTermDoubles : nullptr);
    }
    return cost;
  }
  // residuals and Jacobians: H and g on the device, g and the cost on the host
  int evaluate_full(const double* poses, double* cost) {
    vgx_ctx ctx = pg->ctx;
    const vgx_reg_batch b = with_reg ? pg->batch : nullptr;
    const int m = b ? b->n : 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (m > 0) {
      int rc = vgx_reg_batch_evaluate_normal(b, poses, pg->n_nodes, nullptr, nullptr, nullptr);
      if (rc < 0) return rc;
      rc = vgx_reg_batch_assemble(b, nullptr, pg->n_nodes, pg->d_fused.p, 1);
      if (rc < 0) return rc;
    }
    const double ecost = edge_cost(poses, true);
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      VGX_HIP(ctx, hipSetDevice(ctx->device));
      const size_t E = pg->edges.size();
      if (m > 0) {
        hipLaunchKernelGGL(pg_gather_cost_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, b->d_normal.as<double>(), m,
                           pg->d_cost.get());
        VGX_HIP(ctx, hipMemcpyAsync(h_costs(), pg->d_cost.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      }
      if (E > 0)
        VGX_HIP(ctx, hipMemcpyAsync(pg->d_edge.p, h_edge(), E * kEdgeTermDoubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      if (pg->n_blocks > 0 && pg->lists_sparse)
        hipLaunchKernelGGL(pg_assemble_blocks_tiled_kernel, dim3((pg->n_blocks * 16 + 255) / 256), dim3(256), 0, ctx->stream,
                           pg->d_blocks.get(), pg->d_block_tile.get(), pg->n_blocks, pg->d_block_items.get(), pg->d_fused.get(),
                           pg->d_edge.get(), pg->d_Ht.get());
      else if (pg->n_blocks > 0)
        hipLaunchKernelGGL(pg_assemble_blocks_kernel, dim3((pg->n_blocks * 16 + 255) / 256), dim3(256), 0, ctx->stream, pg->d_blocks.get(),
                           pg->n_blocks, pg->d_block_items.get(), pg->d_fused.get(), pg->d_edge.get(), pg->d_H.get(), pg->nf);
      hipLaunchKernelGGL(pg_assemble_gradient_kernel, dim3((pg->nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_grad_first.get(),
                         pg->d_grad_items.get(), pg->d_fused.get(), pg->d_edge.get(), pg->d_g.get(), pg->nf / 4);
      VGX_HIP(ctx, hipGetLastError());
      VGX_HIP(ctx, hipMemcpyAsync(h_g(), pg->d_g.p, (size_t)pg->nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    double reg = 0.0;
    for (int c = 0; c < m; ++c) reg = reg + h_costs()[c];
    *cost = 0.5 * (reg + ecost);
    reg_seconds += seconds_since(t0);
    ++full_evaluations;
    pg->system_valid = true;
    return VGX_OK;
  }
  int evaluate_cost(const double* poses, double* cost) {
    const vgx_reg_batch b = with_reg ? pg->batch : nullptr;
    const int m = b ? b->n : 0;
    const auto t0 = std::chrono::steady_clock::now();
    double reg = 0.0;
    if (m > 0) {
      const int rc = vgx_reg_batch_evaluate_cost(b, poses, pg->n_nodes, nullptr, h_costs(), nullptr);
      if (rc < 0) return rc;
      for (int c = 0; c < m; ++c) reg = reg + h_costs()[c];
    }
    *cost = 0.5 * (reg + edge_cost(poses, false));
    reg_seconds += seconds_since(t0);
    ++cost_evaluations;
    return VGX_OK;
  }
  // step and H step on the host; *failed: the factorisation met a bad pivot
  int solve_step(double radius, bool* failed) {
    vgx_ctx ctx = pg->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    const int nf = pg->nf;
    std::lock_guard<std::mutex> lk(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    if (pg->lists_sparse) {
      const DeviceTiles& d = pg->tiles;
      hipLaunchKernelGGL(pg_tiles_from_h_kernel, dim3((unsigned)pg->S.l_row.size()), dim3(256), 0, ctx->stream, pg->d_Ht.get(),
                         pg->d_At.get(), d.l_from_h.get());
      hipLaunchKernelGGL(pg_damp_tiled_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_Ht.get(), pg->d_At.get(),
                         d.h_diag.get(), d.col_first.get(), nf, radius);
      int rc = queue_cholesky_tiled(ctx, pg->S, d, pg->d_At.get(), nf, pg->d_flag.get());
      if (rc != VGX_OK) return rc;
      hipLaunchKernelGGL(pg_permute_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_g.get(), d.order.get(),
                         pg->d_x.get(), nf);
      rc = queue_substitutions_tiled(ctx, d, pg->d_At.get(), nf, pg->d_x.get());
      if (rc != VGX_OK) return rc;
      hipLaunchKernelGGL(pg_negate_permuted_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_x.get(), d.order.get(),
                         pg->d_out.get(), nf);
      hipLaunchKernelGGL(pg_matvec_tiled_kernel, dim3((nf + 63) / 64), dim3(64), 0, ctx->stream, pg->d_Ht.get(), d.h_row_first.get(),
                         d.h_col.get(), pg->d_x.get(), d.order.get(), pg->d_out.get(), nf);
      VGX_HIP(ctx, hipGetLastError());
      VGX_HIP(ctx, hipMemcpyAsync(h_step(), pg->d_out.p, 2 * (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      VGX_HIP(ctx, hipMemcpyAsync(h_flag(), pg->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      *failed = *h_flag() != 0;
      la_seconds += seconds_since(t0);
      return VGX_OK;
    }
    VGX_HIP(ctx, hipMemcpyAsync(pg->d_A.p, pg->d_H.p, (size_t)nf * nf * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(pg_damp_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_H.get(), pg->d_A.get(), nf, radius);
    int rc = queue_cholesky(ctx, pg->d_A.get(), nf, pg->d_flag.get());
    if (rc != VGX_OK) return rc;
    VGX_HIP(ctx, hipMemcpyAsync(pg->d_x.p, pg->d_g.p, (size_t)nf * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    rc = queue_substitutions(ctx, pg->d_A.get(), nf, pg->d_x.get());
    if (rc != VGX_OK) return rc;
    hipLaunchKernelGGL(pg_negate_kernel, dim3((nf + 255) / 256), dim3(256), 0, ctx->stream, pg->d_x.get(), pg->d_out.get(), nf);
    hipLaunchKernelGGL(pg_matvec_kernel, dim3((nf + 63) / 64), dim3(64), 0, ctx->stream, pg->d_H.get(), pg->d_out.get(), nf);
    VGX_HIP(ctx, hipGetLastError());
    VGX_HIP(ctx, hipMemcpyAsync(h_step(), pg->d_out.p, 2 * (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipMemcpyAsync(h_flag(), pg->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *failed = *h_flag() != 0;
    la_seconds += seconds_since(t0);
    return VGX_OK;
  }
};

// vgx_dense_spd_solve (m == 0: one right-hand side through the single-column kernels) and vgx_dense_spd_solve_many
// (m > 0: b and x are [n][m]); the entry points have checked the arguments
int dense_spd_solve(vgx_ctx ctx, const char* who_, int32_t n, const double* A, int32_t m, const double* b, double* x, double* L) {
  const std::string who(who_);
  const size_t N = (size_t)n, n_rhs = N * (size_t)std::max(1, m);
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  DeviceArray<double> d_A, d_x;
  DeviceArray<int> d_flag;
  hipError_t e = d_A.alloc_n(N * N);
  if (e == hipSuccess) e = d_x.alloc_n(n_rhs);
  if (e == hipSuccess) e = d_flag.alloc_n(1);
  if (e != hipSuccess) return alloc_error(ctx, e, (who + (m > 0 ? ": allocating the matrix and the right-hand sides" : ": allocating the matrix")).c_str());
  VGX_HIP(ctx, hipMemcpyAsync(d_A.p, A, N * N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  VGX_HIP(ctx, hipMemcpyAsync(d_x.p, b, n_rhs * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  int rc = queue_cholesky(ctx, d_A.get(), n, d_flag.get());
  if (rc == VGX_OK)
    rc = m > 0 ? queue_solve_many(ctx, d_A.get(), n, d_x.get(), m, nullptr, d_flag.get()) : queue_substitutions(ctx, d_A.get(), n, d_x.get());
  if (rc != VGX_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  int flag = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipMemcpyAsync(x, d_x.p, n_rhs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (L) VGX_HIP(ctx, hipMemcpyAsync(L, d_A.p, N * N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (L)
    for (size_t i = 0; i < N; ++i)
      for (size_t j = i + 1; j < N; ++j) L[i * N + j] = 0.0;
  if (flag) return set_error(ctx, VGX_ERR_NOT_POSITIVE_DEFINITE, who + ": the matrix is not positive definite (a pivot is not positive or not finite)");
  return VGX_OK;
}

// What vgx_pose_graph_covariance and vgx_pose_graph_covariance_sparse (`sparse`, with its max_solve_bytes and stats; the
// dense call passes 0 and NULL) check before they plan their columns, in the one order both report in.  Takes pg->mu
// into `lk`.  *go: the caller goes on; else it returns the result (VGX_OK where there is nothing to solve, the
// covariances then written).  *with_reg: the registration batch takes part.  Leaves the index lists made for the call.
int covariance_begin(vgx_pose_graph pg, const char* who_, bool sparse, const double* poses, int32_t exclude_registration_constraints,
                     int32_t n_pairs, const int32_t* pairs, int64_t max_solve_bytes, double* covariance,
                     vgx_pose_graph_covariance_stats* stats, std::unique_lock<std::mutex>& lk, bool* with_reg, bool* go) {
  *go = false;
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  const std::string who(who_);
  if (n_pairs < 0) return set_error(ctx, VGX_ERR_INVALID, who + ": n_pairs < 0");
  if (max_solve_bytes < 0) return set_error(ctx, VGX_ERR_INVALID, who + ": max_solve_bytes < 0");
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n_pairs == 0) return VGX_OK;
  if (!poses || !pairs || !covariance) return set_error(ctx, VGX_ERR_INVALID, who + ": NULL poses, pairs or covariance");
  if (n_pairs > (1 << 26)) return set_error(ctx, VGX_ERR_UNSUPPORTED, who + ": more than 2^26 pairs in one call");
  lk = std::unique_lock<std::mutex>(pg->mu);
  if (sparse && pg->solver != VGX_LINEAR_SOLVER_TILE_SPARSE)
    return set_error(ctx, VGX_ERR_INVALID,
                     who + ": the graph's solver is not VGX_LINEAR_SOLVER_TILE_SPARSE; vgx_pose_graph_covariance takes the dense factor");
  for (size_t i = 0; i < 2 * (size_t)n_pairs; ++i)
    if (pairs[i] < 0 || pairs[i] >= pg->n_nodes)
      return set_error(ctx, VGX_ERR_INVALID, who + ": pair " + std::to_string(i / 2) + " names a node out of range");
  for (size_t i = 0; i < 4 * (size_t)pg->n_nodes; ++i)
    if (!std::isfinite(poses[i])) return set_error(ctx, VGX_ERR_INVALID, who + ": a pose is not finite");
  if (pg->batch) {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    if (pg->batch->destroy_requested) return set_error(ctx, VGX_ERR_INVALID, who + ": the registration batch was destroyed");
  }
  *with_reg = pg->batch && pg->batch->n > 0 && !exclude_registration_constraints;
  if (!*with_reg && pg->edges.empty())
    return set_error(ctx, VGX_ERR_INVALID, who + ": a graph without constraints (no registration batch in use, no edges)");
  if (!sparse && (int)pg->free_nodes.size() > kMaxFreeNodes)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, who + ": " + std::to_string(pg->free_nodes.size()) +
                                                   " free nodes; the covariances take the dense factor, " + std::to_string(kMaxFreeNodes) +
                                                   " free nodes at the most");
  if (pg->nf == 0) {  // every node is constant
    std::fill(covariance, covariance + 16 * (size_t)n_pairs, 0.0);
    return VGX_OK;
  }
  if (!pg->lists_made || pg->lists_with_reg != *with_reg || pg->lists_sparse != sparse) {  // (the dense call: the dense lists, whatever the solver)
    const int rc = make_lists(pg, *with_reg, sparse);
    if (rc != VGX_OK) return rc;
  }
  *go = true;
  return VGX_OK;
}

// The columns a covariance call solves: the distinct second nodes of the pairs between free nodes, four columns each,
// ascending by place(node) -- a free node's position (among the free nodes, or under the order in use), -1 for a
// constant node.  col_of[position] = its first column or -1; m columns; index = [unit_row m][chunk_rows 2 n_chunks], the
// lists pg_unit_columns_kernel and the solve on many right-hand sides take: the row of each column's 1, and per chunk of
// kSolveCols columns {the first row that is not zero, the lowest row any pair wants of them}.  false: out of host memory.
struct CovarianceColumns {
  std::vector<int32_t> col_of, index;
  int m = 0, n_chunks = 0, n_free_pairs = 0;
};
template <class Place>
bool plan_covariance_columns(int nfn, int32_t n_pairs, const int32_t* pairs, Place place, CovarianceColumns* out) try {
  std::vector<int32_t> lowest((size_t)nfn, INT32_MAX);  // per position: the lowest row any of its pairs wants
  out->col_of.assign((size_t)nfn, -1);
  out->m = out->n_free_pairs = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t a = place(pairs[2 * p]), b = place(pairs[2 * p + 1]);
    if (a >= 0 && b >= 0) {
      lowest[(size_t)b] = std::min(lowest[(size_t)b], 4 * a);
      ++out->n_free_pairs;
    }
  }
  for (int b = 0; b < nfn; ++b)
    if (lowest[(size_t)b] != INT32_MAX) {
      out->col_of[(size_t)b] = out->m;
      out->m += 4;
    }
  const int m = out->m, n_chunks = out->n_chunks = (m + kSolveCols - 1) / kSolveCols;
  out->index.assign((size_t)m + 2 * (size_t)n_chunks, INT32_MAX);
  int32_t* unit_row = out->index.data();
  int32_t* chunk_rows = unit_row + m;
  for (int b = 0; b < nfn; ++b) {
    const int c = out->col_of[(size_t)b];
    if (c < 0) continue;
    for (int k = 0; k < 4; ++k) unit_row[c + k] = 4 * b + k;
    int32_t& low = chunk_rows[2 * (c / kSolveCols) + 1];  // (4 | kSolveCols: a node's columns share a chunk)
    low = std::min(low, lowest[(size_t)b]);
  }
  for (int c = 0; c < n_chunks; ++c) chunk_rows[2 * c] = unit_row[c * kSolveCols];  // ascending: the chunk's first 1
  return true;
} catch (const std::bad_alloc&) {
  return false;
}

}  // namespace

extern "C" {

void vgx_pose_graph_options_default(vgx_pose_graph_options* o) {
  if (!o) return;
  o->parameter_tolerance = 3e-3;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->max_solver_time_in_seconds = 4.0;
  o->initial_trust_region_radius = 1e4;
  o->max_num_iterations = 50;
  o->exclude_registration_constraints = 0;
}

int vgx_pose_graph_create(vgx_ctx ctx, int32_t n_nodes, const int32_t* constant, vgx_pose_graph* out) {
  return vgx_pose_graph_create_with_solver(ctx, n_nodes, constant, VGX_LINEAR_SOLVER_DENSE, VGX_ORDER_NATURAL, nullptr, out);
}

int vgx_pose_graph_create_with_solver(vgx_ctx ctx, int32_t n_nodes, const int32_t* constant, int32_t solver, int32_t ordering,
                                      const int32_t* permutation, vgx_pose_graph* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_create: NULL context or output");
  *out = nullptr;
  if (solver != VGX_LINEAR_SOLVER_DENSE && solver != VGX_LINEAR_SOLVER_TILE_SPARSE)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_create: an unknown linear solver");
  if (n_nodes <= 0) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_create: an empty graph (n_nodes <= 0)");
  vgx_pose_graph pg = new (std::nothrow) vgx_pose_graph_s;
  if (!pg) return set_error(ctx, VGX_ERR_NOMEM, "vgx_pose_graph_create: out of host memory");
  pg->ctx = ctx;
  pg->n_nodes = n_nodes;
  pg->pos.assign((size_t)n_nodes, -1);
  for (int i = 0; i < n_nodes; ++i)
    if (constant ? constant[i] == 0 : i != 0) {
      pg->pos[(size_t)i] = (int32_t)pg->free_nodes.size();
      pg->free_nodes.push_back(i);
    }
  if (solver == VGX_LINEAR_SOLVER_DENSE && (int)pg->free_nodes.size() > kMaxFreeNodes) {
    const size_t n_free = pg->free_nodes.size();
    delete pg;
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_pose_graph_create: " + std::to_string(n_free) + " free nodes; the dense solve takes " +
                                                   std::to_string(kMaxFreeNodes) + " at the most");
  }
  if (pg->free_nodes.size() > ((size_t)1 << 27)) {
    delete pg;
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_pose_graph_create: more than 2^27 free nodes");
  }
  pg->nf = 4 * (int)pg->free_nodes.size();
  if (solver != VGX_LINEAR_SOLVER_DENSE || ordering != VGX_ORDER_NATURAL) {
    const int rc = vgx_pose_graph_set_linear_solver(pg, solver, ordering, permutation);
    if (rc != VGX_OK) {
      delete pg;
      return rc;
    }
  }
  *out = pg;
  return VGX_OK;
}

int vgx_pose_graph_set_linear_solver(vgx_pose_graph pg, int32_t solver, int32_t ordering, const int32_t* permutation) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  if (solver != VGX_LINEAR_SOLVER_DENSE && solver != VGX_LINEAR_SOLVER_TILE_SPARSE)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_linear_solver: an unknown linear solver");
  if (ordering != VGX_ORDER_NATURAL && ordering != VGX_ORDER_RCM && ordering != VGX_ORDER_GIVEN)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_linear_solver: an unknown ordering");
  const int32_t nfn = (int32_t)pg->free_nodes.size();
  if (ordering == VGX_ORDER_GIVEN && !is_permutation(permutation, nfn))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_linear_solver: the permutation is NULL or not a permutation of the free nodes");
  if (solver == VGX_LINEAR_SOLVER_DENSE && nfn > kMaxFreeNodes)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_pose_graph_set_linear_solver: " + std::to_string(nfn) + " free nodes; the dense solve takes " +
                                                   std::to_string(kMaxFreeNodes) + " at the most");
  std::lock_guard<std::mutex> lk(pg->mu);
  pg->solver = solver;
  pg->ordering = ordering;
  pg->given_order.clear();
  if (ordering == VGX_ORDER_GIVEN) pg->given_order.assign(permutation, permutation + nfn);
  pg->lists_made = false;
  return VGX_OK;
}

int vgx_pose_graph_structure(vgx_pose_graph pg, vgx_pose_graph_structure_stats* stats) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  if (!stats) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_structure: NULL stats");
  std::lock_guard<std::mutex> lk(pg->mu);
  if (!pg->lists_made || !pg->lists_sparse)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_structure: the tile-sparse solver has made no lists yet (no solve since the last change)");
  stats->n_free_variables = pg->nf;
  stats->n_panels = pg->S.n_tile_rows;
  stats->n_launches = launches_per_factorisation(pg->S);
  stats->reserved = 0;
  stats->n_h_tiles = (int64_t)pg->S.h_col.size();
  stats->n_l_tiles = (int64_t)pg->S.l_row.size();
  stats->n_update_triples = (int64_t)pg->S.triples.size();
  stats->bytes = (int64_t)pg->sparse_bytes;
  return VGX_OK;
}

int vgx_pose_graph_order(vgx_pose_graph pg, int32_t* permutation_out) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  if (!permutation_out) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_order: NULL output");
  std::lock_guard<std::mutex> lk(pg->mu);
  const size_t nfn = pg->free_nodes.size();
  const bool dense = pg->solver == VGX_LINEAR_SOLVER_DENSE;
  if (!dense && pg->ordering == VGX_ORDER_RCM && !(pg->lists_made && pg->lists_sparse))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_order: the RCM order is made with the lists (no solve since the last change)");
  for (size_t i = 0; i < nfn; ++i)
    permutation_out[i] = dense ? (int32_t)i : pg->ordering == VGX_ORDER_RCM ? pg->S.order[i] : pg->ordering == VGX_ORDER_GIVEN ? pg->given_order[i] : (int32_t)i;
  return VGX_OK;
}

int vgx_pose_graph_destroy(vgx_pose_graph pg) {
  if (!pg) return VGX_ERR_INVALID;
  {
    std::lock_guard<std::mutex> lk(pg->ctx->mu);
    (void)hipSetDevice(pg->ctx->device);
    (void)hipStreamSynchronize(pg->ctx->stream);
  }
  release_batch(pg);
  delete pg;
  return VGX_OK;
}

int vgx_pose_graph_set_registration(vgx_pose_graph pg, vgx_reg_batch batch) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  std::lock_guard<std::mutex> lk(pg->mu);
  if (batch) {
    if (batch->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_registration: the batch belongs to another context");
    if (batch->n_global != batch->n)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_registration: a sharded batch (n_global != n); the solve needs the whole list");
    for (int32_t v : batch->node_pair)
      if (v < 0 || v >= pg->n_nodes)
        return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_registration: the batch names a node out of range");
    std::lock_guard<std::mutex> lt(lifetime_mu());
    if (batch->destroy_requested) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_registration: the batch was destroyed");
    ++batch->users;
  }
  release_batch(pg);
  pg->batch = batch;
  pg->lists_made = false;
  return VGX_OK;
}

int vgx_pose_graph_set_edges(vgx_pose_graph pg, int32_t n_edges, const vgx_pose_graph_edge* edges) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  if (n_edges < 0 || (n_edges > 0 && !edges)) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_edges: n_edges < 0 or NULL edges");
  for (int e = 0; e < n_edges; ++e) {
    if (edges[e].a < 0 || edges[e].a >= pg->n_nodes || edges[e].b < 0 || edges[e].b >= pg->n_nodes)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_edges: edge " + std::to_string(e) + " names a node out of range");
    if (edges[e].a == edges[e].b)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_edges: edge " + std::to_string(e) + " joins a node to itself");
    bool finite = std::isfinite(edges[e].yaw_obs);
    for (double v : edges[e].t_obs) finite = finite && std::isfinite(v);
    for (double v : edges[e].sqrt_information) finite = finite && std::isfinite(v);
    if (!finite)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_set_edges: edge " + std::to_string(e) + " has a t_obs, yaw_obs or sqrt_information that is not finite");
  }
  std::lock_guard<std::mutex> lk(pg->mu);
  pg->edges.assign(edges, edges + n_edges);
  pg->lists_made = false;
  return VGX_OK;
}

int vgx_pose_graph_optimize(vgx_pose_graph pg, const vgx_pose_graph_options* options, double* poses, vgx_pose_graph_summary* summary) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  if (!poses) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: NULL poses");
  std::lock_guard<std::mutex> lk(pg->mu);
  vgx_pose_graph_options opt;
  vgx_pose_graph_options_default(&opt);
  if (options) opt = *options;
  vgx_pose_graph_summary S;
  std::memset(&S, 0, sizeof(S));
  S.num_free_nodes = (int32_t)pg->free_nodes.size();
  pg->history.clear();
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < 4 * (size_t)pg->n_nodes; ++i)
    if (!std::isfinite(poses[i])) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: a pose is not finite");
  if (!(opt.initial_trust_region_radius > 0.0))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: initial_trust_region_radius must be positive");
  if (pg->batch) {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    if (pg->batch->destroy_requested)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: the registration batch was destroyed");
  }
  const bool with_reg = pg->batch && pg->batch->n > 0 && !opt.exclude_registration_constraints;
  if (!with_reg && pg->edges.empty())
    return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_optimize: a graph without constraints (no registration batch in use, no edges)");
  if (pg->nf == 0) {  // nothing to optimise
    S.termination_type = VGX_CONVERGENCE;
    S.termination_reason = VGX_TERMINATION_NO_FREE_NODES;
    S.total_seconds = seconds_since(t0);
    if (summary) *summary = S;
    return VGX_OK;
  }
  const bool sparse = pg->solver == VGX_LINEAR_SOLVER_TILE_SPARSE;
  if (!pg->lists_made || pg->lists_with_reg != with_reg || pg->lists_sparse != sparse) {
    const int rc = make_lists(pg, with_reg, sparse);
    if (rc != VGX_OK) return rc;
  }
  Solve sv{pg, with_reg};
  const int n = pg->n_nodes, nf = pg->nf;
  std::vector<double> x(poses, poses + 4 * (size_t)n), cand(4 * (size_t)n), g((size_t)nf);
  double cost = 0.0;
  int rc = sv.evaluate_full(x.data(), &cost);
  if (rc < 0) return rc;
  std::copy(sv.h_g(), sv.h_g() + nf, g.begin());
  S.initial_cost = cost;
  double radius = opt.initial_trust_region_radius, decrease = 2.0;
  int it = 0, reason = VGX_TERMINATION_MAX_ITERATIONS;
  while (it < opt.max_num_iterations) {
    ++it;
    pg->history.push_back(vgx_pose_graph_iteration{cost, 0.0, 0.0, radius, 0.0, 0, 0});
    vgx_pose_graph_iteration& rec = pg->history.back();
    double gmax = 0.0;  // a NaN stays: max |g| of a NaN gradient is a NaN, which is not <= the tolerance
    for (int i = 0; i < nf; ++i) {
      const double a = std::fabs(g[(size_t)i]);
      if (a > gmax || std::isnan(a)) gmax = a;
    }
    if (gmax <= opt.gradient_tolerance) {
      reason = VGX_TERMINATION_GRADIENT_TOLERANCE;
      break;
    }
    bool failed = false;
    rc = sv.solve_step(radius, &failed);
    if (rc < 0) return rc;
    if (failed) {
      rec.factorization_failed = 1;
      ++S.num_factorization_failures;
      radius /= decrease;
      decrease *= 2.0;
      continue;
    }
    const double* step = sv.h_step();
    const double* Hs = sv.h_Hs();
    double s2 = 0.0, x2 = 0.0;
    for (int i = 0; i < nf; ++i) s2 = s2 + step[i] * step[i];
    for (int i = 0; i < nf; ++i) {
      const double v = x[4 * (size_t)pg->free_nodes[(size_t)(i >> 2)] + (i & 3)];
      x2 = x2 + v * v;
    }
    const double step_norm = std::sqrt(s2);
    rec.step_norm = step_norm;
    if (step_norm <= opt.parameter_tolerance * (std::sqrt(x2) + opt.parameter_tolerance)) {
      reason = VGX_TERMINATION_PARAMETER_TOLERANCE;
      break;
    }
    cand = x;
    for (int i = 0; i < nf; ++i) {
      double& v = cand[4 * (size_t)pg->free_nodes[(size_t)(i >> 2)] + (i & 3)];
      v = v + step[i];
    }
    for (int k = 0; k < n; ++k) cand[4 * (size_t)k + 3] = normalize_angle(cand[4 * (size_t)k + 3]);
    double trial = 0.0;
    rc = sv.evaluate_cost(cand.data(), &trial);
    if (rc < 0) return rc;
    double gs = 0.0, sHs = 0.0;
    for (int i = 0; i < nf; ++i) gs = gs + g[(size_t)i] * step[i];
    for (int i = 0; i < nf; ++i) sHs = sHs + step[i] * Hs[i];
    const double model_decrease = -(gs + 0.5 * sHs);
    const double rho = model_decrease > 0.0 ? (cost - trial) / model_decrease : -1.0;
    rec.trial_cost = trial;
    rec.gain_ratio = rho;
    if (rho > 1e-3) {
      rec.accepted = 1;
      ++S.num_successful_steps;
      double new_cost = 0.0;
      rc = sv.evaluate_full(cand.data(), &new_cost);
      if (rc < 0) return rc;
      const double rel = std::fabs(cost - new_cost) / std::max(cost, 1e-300);
      x = cand;
      cost = new_cost;
      std::copy(sv.h_g(), sv.h_g() + nf, g.begin());
      const double q = 2.0 * rho - 1.0;
      radius = std::min(radius / std::max(1.0 / 3.0, 1.0 - q * q * q), 1e16);
      decrease = 2.0;
      if (rel <= opt.function_tolerance) {
        reason = VGX_TERMINATION_FUNCTION_TOLERANCE;
        break;
      }
    } else {
      radius /= decrease;
      decrease *= 2.0;
    }
    if (seconds_since(t0) > opt.max_solver_time_in_seconds) {
      reason = VGX_TERMINATION_MAX_SOLVER_TIME;
      break;
    }
  }
  std::copy(x.begin(), x.end(), poses);
  S.termination_reason = reason;
  S.termination_type = reason <= VGX_TERMINATION_GRADIENT_TOLERANCE ? VGX_CONVERGENCE : VGX_NO_CONVERGENCE;
  S.num_iterations = it;
  S.num_full_evaluations = sv.full_evaluations;
  S.num_cost_evaluations = sv.cost_evaluations;
  S.final_cost = cost;
  S.registration_seconds = sv.reg_seconds;
  S.linear_algebra_seconds = sv.la_seconds;
  S.total_seconds = seconds_since(t0);
  if (summary) *summary = S;
  return VGX_OK;
}

int vgx_pose_graph_history(vgx_pose_graph pg, int32_t capacity, vgx_pose_graph_iteration* iterations, int32_t* n_iterations) {
  if (!pg) return VGX_ERR_INVALID;
  if (capacity < 0 || (capacity > 0 && !iterations))
    return set_error(pg->ctx, VGX_ERR_INVALID, "vgx_pose_graph_history: capacity < 0 or NULL iterations");
  std::lock_guard<std::mutex> lk(pg->mu);
  if (n_iterations) *n_iterations = (int32_t)pg->history.size();
  const size_t k = std::min(pg->history.size(), (size_t)capacity);
  if (k) std::memcpy(iterations, pg->history.data(), k * sizeof(vgx_pose_graph_iteration));
  return VGX_OK;
}

int vgx_pose_graph_download_system(vgx_pose_graph pg, int32_t* n_free_variables, double* H, double* g) {
  if (!pg) return VGX_ERR_INVALID;
  vgx_ctx ctx = pg->ctx;
  std::lock_guard<std::mutex> lk(pg->mu);
  if (n_free_variables) *n_free_variables = pg->nf;
  if (!H && !g) return VGX_OK;
  if (!pg->system_valid) return set_error(ctx, VGX_ERR_INVALID, "vgx_pose_graph_download_system: no solve has evaluated the system yet");
  const size_t nf = (size_t)pg->nf;
  std::lock_guard<std::mutex> lc(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (g) VGX_HIP(ctx, hipMemcpy(g, pg->d_g.p, nf * sizeof(double), hipMemcpyDeviceToHost));
  if (H && pg->lists_sparse) {  // the tiles scattered to the dense matrix, in ascending node order whatever the order in use
    if (nf > (size_t)kMaxDenseN)
      return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_pose_graph_download_system: the dense H of " + std::to_string(nf) +
                                                     " free variables is not made (" + std::to_string(kMaxDenseN) + " at the most); g is delivered");
    const TileStructure& S = pg->S;
    std::vector<double> tiles;
    try {
      tiles.resize(S.h_col.size() * (size_t)kTileDoubles);
    } catch (const std::bad_alloc&) {
      return set_error(ctx, VGX_ERR_NOMEM, "vgx_pose_graph_download_system: out of host memory for the tiles of H");
    }
    VGX_HIP(ctx, hipMemcpy(tiles.data(), pg->d_Ht.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::fill(H, H + nf * nf, 0.0);
    for (int32_t I = 0; I < S.n_tile_rows; ++I)
      for (int32_t t = S.h_row_first[(size_t)I]; t < S.h_row_first[(size_t)I + 1]; ++t) {
        const int32_t J = S.h_col[(size_t)t];
        for (int r = 0; r < S.rows_of(I); ++r)
          for (int c = 0; c < S.rows_of(J); ++c) {
            const size_t row = 4 * (size_t)S.order[(size_t)(I * kNodesPerTile + r / 4)] + r % 4;
            const size_t col = 4 * (size_t)S.order[(size_t)(J * kNodesPerTile + c / 4)] + c % 4;
            H[row * nf + col] = tiles[(size_t)t * kTileDoubles + r * kPanel + c];
          }
      }
  } else if (H) {
    VGX_HIP(ctx, hipMemcpy(H, pg->d_H.p, nf * nf * sizeof(double), hipMemcpyDeviceToHost));
  }
  return VGX_OK;
}

int vgx_dense_spd_solve(vgx_ctx ctx, int32_t n, const double* A, const double* b, double* x, double* L) {
  if (!ctx) return VGX_ERR_INVALID;
  if (n < 1 || n > kMaxDenseN)
    return set_error(ctx, n < 1 ? VGX_ERR_INVALID : VGX_ERR_UNSUPPORTED, "vgx_dense_spd_solve: n must be in [1, " + std::to_string(kMaxDenseN) + "]");
  if (!A || !b || !x) return set_error(ctx, VGX_ERR_INVALID, "vgx_dense_spd_solve: NULL A, b or x");
  return dense_spd_solve(ctx, "vgx_dense_spd_solve", n, A, 0, b, x, L);
}

int vgx_pose_graph_covariance(vgx_pose_graph pg, const double* poses, int32_t exclude_registration_constraints, int32_t n_pairs,
                              const int32_t* pairs, double* covariance) {
  std::unique_lock<std::mutex> lk;
  bool with_reg = false, go = false;
  int rc = covariance_begin(pg, "vgx_pose_graph_covariance", false, poses, exclude_registration_constraints, n_pairs, pairs, 0, covariance,
                            nullptr, lk, &with_reg, &go);
  if (!go) return rc;
  vgx_ctx ctx = pg->ctx;
  // the columns to solve, in ascending free position
  const int nf = pg->nf;
  CovarianceColumns cols;
  if (!plan_covariance_columns(nf / 4, n_pairs, pairs, [&](int32_t node) { return pg->pos[(size_t)node]; }, &cols))
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_pose_graph_covariance: out of host memory for the column lists");
  const std::vector<int32_t>& col_of = cols.col_of;
  const int m = cols.m, n_chunks = cols.n_chunks;
  const size_t n_out = 16 * (size_t)n_pairs, n_index = cols.index.size() + 2 * (size_t)n_pairs;
  {
    std::lock_guard<std::mutex> lc(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = pg->d_X.reserve(std::max<size_t>(1, (size_t)nf * m) * sizeof(double));
    if (e == hipSuccess) e = pg->d_cov.reserve((n_out + 1) * sizeof(double));
    if (e == hipSuccess) e = pg->d_cov_index.reserve(n_index * sizeof(int32_t));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_pose_graph_covariance: allocating the solved columns");
    e = pg->h_cov.reserve((n_out + 1) * sizeof(double) + n_index * sizeof(int32_t));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_pose_graph_covariance: allocating the pinned staging");
  }
  double* h_out = pg->h_cov.as<double>();
  int32_t* h_unit_row = reinterpret_cast<int32_t*>(h_out + n_out + 1);  // [unit_row m][chunk_rows 2 n_chunks][block 2 n_pairs]
  std::copy(cols.index.begin(), cols.index.end(), h_unit_row);
  int32_t* h_block = h_unit_row + cols.index.size();
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t a = pg->pos[(size_t)pairs[2 * p]], b = pg->pos[(size_t)pairs[2 * p + 1]];
    h_block[2 * p] = a >= 0 ? 4 * a : -1;
    h_block[2 * p + 1] = b >= 0 ? col_of[(size_t)b] : -1;
    if (a < 0) h_block[2 * p + 1] = -1;
  }
  Solve sv{pg, with_reg};
  double cost = 0.0;
  rc = sv.evaluate_full(poses, &cost);
  if (rc < 0) return rc;
  {
    std::lock_guard<std::mutex> lc(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    int32_t* d_unit_row = pg->d_cov_index.get();
    int32_t* d_chunk_rows = d_unit_row + m;
    int32_t* d_block = d_chunk_rows + 2 * (size_t)n_chunks;
    VGX_HIP(ctx, hipMemcpyAsync(d_unit_row, h_unit_row, n_index * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    VGX_HIP(ctx, hipMemcpyAsync(pg->d_A.p, pg->d_H.p, (size_t)nf * nf * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    rc = queue_cholesky(ctx, pg->d_A.get(), nf, pg->d_flag.get());  // undamped
    if (rc != VGX_OK) return rc;
    if (m > 0) {
      const size_t total = (size_t)nf * m;
      hipLaunchKernelGGL(pg_unit_columns_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, pg->d_X.get(), nf, m,
                         d_unit_row);
      rc = queue_solve_many(ctx, pg->d_A.get(), nf, pg->d_X.get(), m, d_chunk_rows, pg->d_flag.get());
      if (rc != VGX_OK) return rc;
    }
    hipLaunchKernelGGL(pg_gather_blocks_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, ctx->stream, pg->d_X.get(), m, d_block,
                       n_pairs, pg->d_flag.get(), pg->d_cov.get());
    VGX_HIP(ctx, hipGetLastError());
    VGX_HIP(ctx, hipMemcpyAsync(h_out, pg->d_cov.p, (n_out + 1) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (h_out[n_out] != 0.0)
    return set_error(ctx, VGX_ERR_NOT_POSITIVE_DEFINITE,
                     "vgx_pose_graph_covariance: H is not positive definite (a pivot is not positive or not finite): the graph is rank deficient");
  std::memcpy(covariance, h_out, n_out * sizeof(double));
  return VGX_OK;
}

int vgx_pose_graph_covariance_sparse(vgx_pose_graph pg, const double* poses, int32_t exclude_registration_constraints, int32_t n_pairs,
                                     const int32_t* pairs, int64_t max_solve_bytes, double* covariance,
                                     vgx_pose_graph_covariance_stats* stats) {
  std::unique_lock<std::mutex> lk;
  bool with_reg = false, go = false;
  int rc = covariance_begin(pg, "vgx_pose_graph_covariance_sparse", true, poses, exclude_registration_constraints, n_pairs, pairs,
                            max_solve_bytes, covariance, stats, lk, &with_reg, &go);
  if (!go) return rc;
  vgx_ctx ctx = pg->ctx;
  // the columns to solve, in ascending POSITION under the order in use
  const int nf = pg->nf;
  const std::vector<int32_t>& position = pg->S.position;
  auto place = [&](int32_t node) { return pg->pos[(size_t)node] < 0 ? -1 : position[(size_t)pg->pos[(size_t)node]]; };
  CovarianceColumns cols;
  if (!plan_covariance_columns(nf / 4, n_pairs, pairs, place, &cols))
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_pose_graph_covariance_sparse: out of host memory for the column lists");
  const std::vector<int32_t>& col_of = cols.col_of;
  const int m = cols.m;
  const size_t n_out = 16 * (size_t)n_pairs;
  std::vector<int32_t> slab_first;
  // the slabs: S columns at a time, the largest multiple of kSolveCols with 8 nf S <= the budget, kSolveCols at the least
  const int64_t budget = max_solve_bytes == 0 ? (int64_t)1 << 30 : max_solve_bytes;
  const int64_t m_round = ((int64_t)m + kSolveCols - 1) / kSolveCols * kSolveCols;
  const int64_t slab = std::max<int64_t>(kSolveCols, std::min<int64_t>(std::max<int64_t>(m_round, kSolveCols), budget / (8 * (int64_t)nf) / kSolveCols * kSolveCols));
  const int n_slabs = (int)((m + slab - 1) / slab), n_chunks = cols.n_chunks;
  const size_t x_doubles = (size_t)nf * (size_t)std::min<int64_t>(slab, std::max(m, 1));
  const size_t x_limit = std::max<size_t>((size_t)budget, (size_t)nf * kSolveCols * sizeof(double));
  const size_t n_index = cols.index.size() + 3 * (size_t)cols.n_free_pairs + 1;
  {
    std::lock_guard<std::mutex> lc(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    if (pg->d_X.bytes < x_doubles * sizeof(double) || pg->d_X.bytes > x_limit) {  // grown on demand, never past the budget
      VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      e = pg->d_X.alloc(x_doubles * sizeof(double));
    }
    if (e == hipSuccess) e = pg->d_cov.reserve((n_out + 1) * sizeof(double));
    if (e == hipSuccess) e = pg->d_cov_index.reserve(n_index * sizeof(int32_t));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_pose_graph_covariance_sparse: allocating the solved columns");
    e = pg->h_cov.reserve((n_out + 1) * sizeof(double) + n_index * sizeof(int32_t));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_pose_graph_covariance_sparse: allocating the pinned staging");
  }
  double* h_out = pg->h_cov.as<double>();
  int32_t* h_unit_row = reinterpret_cast<int32_t*>(h_out + n_out + 1);  // [unit_row m][chunk_rows 2 n_chunks][the slabs' pairs]
  std::copy(cols.index.begin(), cols.index.end(), h_unit_row);
  int32_t* h_list = h_unit_row + cols.index.size();  // per slab its pairs: {pair, first row, first column in the slab}
  try {
    slab_first.assign((size_t)n_slabs + 1, 0);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_pose_graph_covariance_sparse: out of host memory for the column lists");
  }
  for (int pass = 0; pass < 2; ++pass) {  // a counting sort of the pairs by slab, stable
    for (int p = 0; p < n_pairs; ++p) {
      const int32_t a = place(pairs[2 * p]), b = place(pairs[2 * p + 1]);
      if (a < 0 || b < 0) continue;
      const int32_t col = col_of[(size_t)b], s = (int32_t)(col / slab);
      if (pass == 0) {
        ++slab_first[(size_t)s + 1];
      } else {
        int32_t* rec = h_list + 3 * (size_t)slab_first[(size_t)s]++;
        rec[0] = p, rec[1] = 4 * a, rec[2] = (int32_t)(col - s * slab);
      }
    }
    if (pass == 0)
      for (int s = 0; s < n_slabs; ++s) slab_first[(size_t)s + 1] += slab_first[(size_t)s];
    else
      for (int s = n_slabs; s > 0; --s) slab_first[(size_t)s] = slab_first[(size_t)s - 1];
    if (pass == 1) slab_first[0] = 0;
  }
  Solve sv{pg, with_reg};
  double cost = 0.0;
  rc = sv.evaluate_full(poses, &cost);
  if (rc < 0) return rc;
  {
    std::lock_guard<std::mutex> lc(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    const DeviceTiles& d = pg->tiles;
    int32_t* d_unit_row = pg->d_cov_index.get();
    int32_t* d_chunk_rows = d_unit_row + m;
    int32_t* d_list = d_chunk_rows + 2 * (size_t)n_chunks;
    VGX_HIP(ctx, hipMemcpyAsync(d_unit_row, h_unit_row, n_index * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    VGX_HIP(ctx, hipMemsetAsync(pg->d_cov.p, 0, n_out * sizeof(double), ctx->stream));  // a pair with a constant node: zeros
    hipLaunchKernelGGL(pg_tiles_from_h_kernel, dim3((unsigned)pg->S.l_row.size()), dim3(256), 0, ctx->stream, pg->d_Ht.get(),
                       pg->d_At.get(), d.l_from_h.get());
    rc = queue_cholesky_tiled(ctx, pg->S, d, pg->d_At.get(), nf, pg->d_flag.get());  // undamped
    if (rc != VGX_OK) return rc;
    for (int s = 0; s < n_slabs; ++s) {
      const int64_t c_first = s * slab;
      const int ms = (int)std::min<int64_t>(slab, m - c_first);
      const size_t total = (size_t)nf * ms;
      hipLaunchKernelGGL(pg_unit_columns_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, pg->d_X.get(), nf, ms,
                         d_unit_row + c_first);
      rc = queue_solve_many_tiled(ctx, d, pg->d_At.get(), nf, pg->d_X.get(), ms, d_chunk_rows + 2 * (c_first / kSolveCols), pg->d_flag.get());
      if (rc != VGX_OK) return rc;
      const int n_list = slab_first[(size_t)s + 1] - slab_first[(size_t)s];  // (> 0: every column has a pair that wants it)
      hipLaunchKernelGGL(pg_gather_slab_blocks_kernel, dim3((unsigned)(((size_t)n_list * 16 + 255) / 256)), dim3(256), 0, ctx->stream,
                         pg->d_X.get(), ms, d_list + 3 * (size_t)slab_first[(size_t)s], n_list, pg->d_cov.get());
    }
    VGX_HIP(ctx, hipGetLastError());
    VGX_HIP(ctx, hipMemcpyAsync(h_out, pg->d_cov.p, n_out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipMemcpyAsync(h_out + n_out, pg->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (stats) {
    stats->n_columns = m;
    stats->n_slabs = n_slabs;
    stats->n_launches = 1 + launches_per_factorisation(pg->S) + 4 * n_slabs;
    stats->reserved = 0;
    stats->solve_bytes = m > 0 ? (int64_t)(x_doubles * sizeof(double)) : 0;
  }
  if (*reinterpret_cast<const int*>(h_out + n_out) != 0)
    return set_error(ctx, VGX_ERR_NOT_POSITIVE_DEFINITE,
                     "vgx_pose_graph_covariance_sparse: H is not positive definite (a pivot is not positive or not finite): the graph is rank deficient");
  std::memcpy(covariance, h_out, n_out * sizeof(double));
  return VGX_OK;
}

int vgx_dense_spd_solve_many(vgx_ctx ctx, int32_t n, const double* A, int32_t m, const double* B, double* X, double* L) {
  if (!ctx) return VGX_ERR_INVALID;
  if (n < 1 || n > kMaxDenseN || m < 1 || m > kMaxDenseN)
    return set_error(ctx, (n < 1 || m < 1) ? VGX_ERR_INVALID : VGX_ERR_UNSUPPORTED,
                     "vgx_dense_spd_solve_many: n and m must be in [1, " + std::to_string(kMaxDenseN) + "]");
  if (!A || !B || !X) return set_error(ctx, VGX_ERR_INVALID, "vgx_dense_spd_solve_many: NULL A, B or X");
  return dense_spd_solve(ctx, "vgx_dense_spd_solve_many", n, A, m, B, X, L);
}

int vgx_block_spd_solve(vgx_ctx ctx, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj, const double* values,
                        const double* b, double* x, vgx_pose_graph_structure_stats* stats, int32_t* tile_index, double* tile_values) {
  if (!ctx) return VGX_ERR_INVALID;
  if (n_block_rows < 1 || nnz < 1) return set_error(ctx, VGX_ERR_INVALID, "vgx_block_spd_solve: n_block_rows < 1 or nnz < 1");
  if (n_block_rows > (1 << 27)) return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_block_spd_solve: more than 2^27 block rows");
  if (!bi || !bj || !values || !b || !x) return set_error(ctx, VGX_ERR_INVALID, "vgx_block_spd_solve: NULL bi, bj, values, b or x");
  try {
    return block_spd_solve(ctx, "vgx_block_spd_solve", n_block_rows, nnz, bi, bj, values, 0, b, x, stats, tile_index, tile_values);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_block_spd_solve: out of host memory for the structure or the tiles");
  }
}

int vgx_block_spd_solve_many(vgx_ctx ctx, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj, const double* values,
                             int32_t m, const double* B, double* X) {
  if (!ctx) return VGX_ERR_INVALID;
  if (n_block_rows < 1 || nnz < 1 || m < 1) return set_error(ctx, VGX_ERR_INVALID, "vgx_block_spd_solve_many: n_block_rows < 1, nnz < 1 or m < 1");
  if (n_block_rows > (1 << 27)) return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_block_spd_solve_many: more than 2^27 block rows");
  if (m > kMaxDenseN) return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_block_spd_solve_many: m must be in [1, " + std::to_string(kMaxDenseN) + "]");
  if (!bi || !bj || !values || !B || !X) return set_error(ctx, VGX_ERR_INVALID, "vgx_block_spd_solve_many: NULL bi, bj, values, B or X");
  try {
    return block_spd_solve(ctx, "vgx_block_spd_solve_many", n_block_rows, nnz, bi, bj, values, m, B, X, nullptr, nullptr, nullptr);
  } catch (const std::bad_alloc&) {
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_block_spd_solve_many: out of host memory for the structure or the tiles");
  }
}

}  // extern "C"

namespace {
int block_spd_solve(vgx_ctx ctx, const char* who_, int32_t n_block_rows, int32_t nnz, const int32_t* bi, const int32_t* bj,
                    const double* values, int32_t m, const double* b, double* x, vgx_pose_graph_structure_stats* stats,
                    int32_t* tile_index, double* tile_values) {
  const std::string who(who_);
  std::vector<int32_t> joined(2 * (size_t)nnz);
  std::set<std::pair<int32_t, int32_t>> seen;
  for (int32_t k = 0; k < nnz; ++k) {
    if (bi[k] < 0 || bi[k] >= n_block_rows || bj[k] < 0 || bj[k] >= n_block_rows)
      return set_error(ctx, VGX_ERR_INVALID, who + ": block " + std::to_string(k) + " is out of range");
    if (bj[k] > bi[k]) return set_error(ctx, VGX_ERR_INVALID, who + ": block " + std::to_string(k) + " lies above the diagonal");
    if (!seen.insert({bi[k], bj[k]}).second)
      return set_error(ctx, VGX_ERR_INVALID, who + ": block " + std::to_string(k) + " is given twice");
    joined[2 * (size_t)k] = bi[k];
    joined[2 * (size_t)k + 1] = bj[k];
  }
  TileStructure S;
  if (!build_tile_structure(n_block_rows, nnz, joined.data(), kOrderNatural, nullptr, &S))
    return set_error(ctx, VGX_ERR_INVALID, who + ": the block list does not make a structure");
  const size_t n_l = S.l_row.size(), N = 4 * (size_t)n_block_rows;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = check_tile_cap(ctx, who_, n_l, 0, (N * (size_t)std::max(1, m) + 64) * sizeof(double));
  if (rc != VGX_OK) return rc;
  std::vector<double> tiles(n_l * (size_t)kTileDoubles, 0.0);
  for (int32_t k = 0; k < nnz; ++k) {
    double* T = tiles.data() + (size_t)S.l_tile(bi[k] / kNodesPerTile, bj[k] / kNodesPerTile) * kTileDoubles;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c)
        T[(4 * (bi[k] % kNodesPerTile) + r) * kPanel + 4 * (bj[k] % kNodesPerTile) + c] = values[16 * (size_t)k + 4 * r + c];
  }
  DeviceTiles d;
  DeviceArray<double> d_At, d_x;
  DeviceArray<int> d_flag;
  rc = upload_structure(ctx, S, &d);
  if (rc != VGX_OK) return rc;
  hipError_t e = d_At.alloc_n(n_l * (size_t)kTileDoubles);
  if (e == hipSuccess) e = d_x.alloc_n(N * (size_t)std::max(1, m));
  if (e == hipSuccess) e = d_flag.alloc_n(1);
  if (e != hipSuccess) return alloc_error(ctx, e, (who + ": allocating the tiles").c_str());
  VGX_HIP(ctx, hipMemcpyAsync(d_At.p, tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  VGX_HIP(ctx, hipMemcpyAsync(d_x.p, b, N * (size_t)std::max(1, m) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  rc = queue_cholesky_tiled(ctx, S, d, d_At.get(), (int)N, d_flag.get());
  if (rc == VGX_OK)
    rc = m > 0 ? queue_solve_many_tiled(ctx, d, d_At.get(), (int)N, d_x.get(), m, nullptr, d_flag.get())
               : queue_substitutions_tiled(ctx, d, d_At.get(), (int)N, d_x.get());
  if (rc != VGX_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  int flag = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipMemcpyAsync(x, d_x.p, N * (size_t)std::max(1, m) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (tile_values) VGX_HIP(ctx, hipMemcpyAsync(tile_values, d_At.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (tile_index)
    for (size_t t = 0; t < n_l; ++t) {
      tile_index[2 * t] = S.l_row[t];
      tile_index[2 * t + 1] = S.l_col[t];
    }
  if (tile_values)  // a diagonal tile above its diagonal, and the rows and columns past n: zeros
    for (size_t t = 0; t < n_l; ++t)
      for (int r = 0; r < kPanel; ++r)
        for (int c = 0; c < kPanel; ++c)
          if (r >= S.rows_of(S.l_row[t]) || c >= S.rows_of(S.l_col[t]) || (S.l_row[t] == S.l_col[t] && c > r))
            tile_values[t * kTileDoubles + r * kPanel + c] = 0.0;
  if (stats) {
    stats->n_free_variables = (int32_t)N;
    stats->n_panels = S.n_tile_rows;
    stats->n_launches = launches_per_factorisation(S);
    stats->reserved = 0;
    stats->n_h_tiles = 0;
    for (int32_t v : S.l_from_h) stats->n_h_tiles += v >= 0;
    stats->n_l_tiles = (int64_t)n_l;
    stats->n_update_triples = (int64_t)S.triples.size();
    stats->bytes = (int64_t)(tiles.size() * sizeof(double) + d.bytes);
  }
  if (flag) return set_error(ctx, VGX_ERR_NOT_POSITIVE_DEFINITE, who + ": the matrix is not positive definite (a pivot is not positive or not finite)");
  return VGX_OK;
}
}  // namespace
