// dq_corrmat.hip -- every pairwise Correlation state of k <= 64 numeric columns in one pass over the
// rows (dq_corrmat_*, include/deequ_amd.h), on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).
//
// The sums, slabs, shifts and the fall-back rule are stated in dq_corrmat.h.  The kernel:
//
//  * A workgroup (4 waves) owns a contiguous range of slabs and walks a slab in chunks of 64 rows
//    (16 of them; up to 24 in a batch's last slab, which takes a tail shorter than half a slab).
//  * Staging: wave w loads the chunk of the columns w, w + 4, ... with one row per lane (512
//    contiguous bytes per load), finds the column's shift on its first chunk of the slab that has a
//    selected finite value (a ballot), and writes d_i(r) to LDS column-major, Dt[i][r], with rows of
//    66 doubles, and the chunk's selection of the column as one 64-bit word vm[i].  The writes are
//    contiguous; an MFMA operand read takes lane l's double at Dt[16 t + (l & 15)][4 s + (l >> 4)],
//    whose bank pair is 4 (l & 15) + 2 (l >> 4) + const (mod 64): no two lanes of a 32-lane half
//    share a bank.
//  * Sums: the 16 x 16 tiles (ti <= tj) of the matrix are dealt round robin to the waves; a tile's
//    sums are rank-4 updates C += A B with A[i][r] = Dt[16 ti + i][r], B[r][j] = Dt[16 tj + j][r]
//    (lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; C[(l >> 4) + 4 g][l & 15] in register g).
//      masked (a validity bitmap on a selected column, or a `where`): six products per tile, of d, d²
//        and v (a bit of vm as a double), so a lane ends up with all six sums of its four pairs;
//      fast (every row selected): d_i d_j alone, plus per row-tile one product of d with a column of
//        ones (Σ d_i); Σ d_i² is the diagonal of d_i d_j.  The two go through LDS at the slab's end.
//  * Slab end: every lane folds its pairs' sums into the range's running states (corr_fold_slab),
//    which live in HBM as partials[range][pair] (up to 100 KB per workgroup: too much for LDS
//    next to the stage), or raises the pair's flag.
//  * dq_corrmat_reduce_kernel merges a pair's range states in dq_corr_reduce_kernel's fixed tree.
//  * dq_corrmat_rows_kernel answers the pairs whose sums of finite values overflowed, row by row.
//
// Registers: 4 tiles x 4 doubles (fast), 3 tiles x 6 products x 4 doubles (masked) of accumulators
// per lane.  LDS: 33.8 KB of stage + 1.5 KB of words, shifts and sums per workgroup.
#include "dq_internal.h"
#include "dq_corrmat.h"

namespace dq {

namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kCmStride = kCorrmatChunkRows + 2;  // doubles per LDS row: = 2 (mod 32)
constexpr int kCmSteps = kCorrmatChunkRows / 4;   // MFMA steps per chunk
constexpr int kCmChunks = kCorrmatSlabRows / kCorrmatChunkRows;

constexpr int kCmPerWave = kCorrmatMaxCols / 4;  // columns a wave stages

// A value's bits, and the cast Correlation applies to every numeric type (dq_pair.hip's as_double),
// in two steps: the chunk's loads are issued together and converted when they are used.
__device__ inline uint64_t cm_load_raw(const DevColumn& c, int64_t row) {
  switch (c.type) {
    case DQ_T_INT8: return (uint64_t)(int64_t)static_cast<const int8_t*>(c.values)[row];
    case DQ_T_INT16: return (uint64_t)(int64_t)static_cast<const int16_t*>(c.values)[row];
    case DQ_T_INT32: return (uint64_t)(int64_t)static_cast<const int32_t*>(c.values)[row];
    case DQ_T_FLOAT32: return (uint64_t)static_cast<const uint32_t*>(c.values)[row];
    default: return static_cast<const uint64_t*>(c.values)[row];  // int64, float64
  }
}
__device__ inline double cm_to_double(int type, uint64_t raw) {
  switch (type) {
    case DQ_T_INT8:
    case DQ_T_INT16:
    case DQ_T_INT32:
    case DQ_T_INT64: return (double)(int64_t)raw;
    case DQ_T_FLOAT32: return (double)__builtin_bit_cast(float, (uint32_t)raw);
    default: return __builtin_bit_cast(double, raw);
  }
}

__device__ inline f64x4 cm_mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ inline double cm_pick(const f64x4& v, int g) {
  return g == 0 ? v[0] : g == 1 ? v[1] : g == 2 ? v[2] : v[3];
}

}  // namespace

// blockIdx.x = row range.  sel[0 .. k): the matrix's columns among cols.  partials[range][pair].
template <bool MASKED>
__global__ __launch_bounds__(kBlock) void dq_corrmat_kernel(const DevColumn* __restrict__ cols,
                                                            const int32_t* __restrict__ sel, int k,
                                                            const uint64_t* __restrict__ where_t, int64_t n_rows,
                                                            int64_t slabs_per_range, CorrAcc* __restrict__ partials,
                                                            uint32_t* __restrict__ pair_flags,
                                                            uint32_t* __restrict__ col_flags) {
  constexpr int kSlots = MASKED ? 3 : 4;  // tiles per wave: 10 of 4 x 4 (masked), + 4 of ones (fast)
  constexpr int kProducts = MASKED ? 6 : 1;
  __shared__ double Dt[kCorrmatMaxCols * kCmStride];
  __shared__ unsigned long long vm[kCorrmatMaxCols];
  __shared__ double shift[kCorrmatMaxCols];
  __shared__ int has_shift[kCorrmatMaxCols];
  __shared__ double col_sum[kCorrmatMaxCols], col_sq[kCorrmatMaxCols];  // (fast)

  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int T = (k + 15) >> 4, kp = T << 4;
  const int64_t n_pairs = corrmat_pairs(k);
  const int n_tiles = T * (T + 1) / 2 + (MASKED ? 0 : T);

  // this wave's tiles: (ti, tj), tj == T: the column of ones
  int s_ti[kSlots], s_tj[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int q = wave + 4 * s;
    int ti = -1, tj = -1, at = 0;
    for (int a = 0; a < T; ++a)
      for (int b = a; b < T + (MASKED ? 0 : 1); ++b) {
        if (at == q) {
          ti = a;
          tj = b;
        }
        ++at;
      }
    s_ti[s] = q < n_tiles ? ti : -1;
    s_tj[s] = tj;
  }

  const int64_t n_slabs = corrmat_n_slabs(n_rows);
  const int64_t slab0 = (int64_t)blockIdx.x * slabs_per_range;
  const int64_t slab1 = slab0 + slabs_per_range < n_slabs ? slab0 + slabs_per_range : n_slabs;
  const int64_t end_row = corrmat_slab_end(slab1 - 1, n_slabs, n_rows);
  const int64_t chunk0 = slab0 * kCmChunks;
  const int64_t chunk1 = (end_row + kCorrmatChunkRows - 1) / kCorrmatChunkRows;
  CorrAcc* my = partials + (int64_t)blockIdx.x * n_pairs;

  // A chunk of this wave's columns w, w + 4, ... as raw bits (and validity bytes), one row per lane:
  // loaded a chunk ahead, so that the loads are in flight while the matrix cores run.
  uint64_t raw[kCmPerWave];
  uint32_t vbyte[kCmPerWave];
  unsigned long long wsel = ~0ull;
  auto load_chunk = [&](int64_t chunk) {
    const int64_t row = chunk * kCorrmatChunkRows + lane;
    const bool in = row < end_row;
    if (MASKED && where_t) wsel = where_t[chunk];
#pragma unroll
    for (int u = 0; u < kCmPerWave; ++u) {
      const int ci = wave + 4 * u;
      raw[u] = 0;
      vbyte[u] = 0xffu;
      if (ci < k && in) {
        const DevColumn& col = cols[sel[ci]];
        raw[u] = cm_load_raw(col, row);
        if (MASKED && col.validity) vbyte[u] = col.validity[row >> 3];
      }
    }
  };

  f64x4 acc[kSlots][kProducts];
  if (chunk0 < chunk1) load_chunk(chunk0);
  for (int64_t chunk = chunk0; chunk < chunk1; ++chunk) {
    const int64_t slab = chunk / kCmChunks < n_slabs ? chunk / kCmChunks : n_slabs - 1;  // (the last one takes a short tail)
    const bool slab_first = chunk == slab * kCmChunks;
    const int64_t r0 = chunk * kCorrmatChunkRows;
    const int64_t row = r0 + lane;
    const bool in = row < end_row;
    const bool slab_end = chunk == chunk1 - 1 || ((chunk + 1) / kCmChunks == slab + 1 && slab + 1 < n_slabs);
    if (slab_first) {
#pragma unroll
      for (int s = 0; s < kSlots; ++s)
#pragma unroll
        for (int p = 0; p < kProducts; ++p) acc[s][p] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();  // the last chunk's operands (and the last slab's shifts) have been read
#pragma unroll
    for (int u = 0; u < kCmPerWave; ++u) {
      const int ci = wave + 4 * u;
      if (ci >= kp) continue;  // (wave-uniform)
      double dv = 0.0;
      unsigned long long m = 0ull;
      if (ci < k) {
        if (slab_first) has_shift[ci] = 0;
        bool on = in;
        if (MASKED) on = on && ((wsel >> lane) & 1ull) && ((vbyte[u] >> (row & 7)) & 1u);
        const double x = cm_to_double(cols[sel[ci]].type, raw[u]);
        const bool fin = corrmat_finite(x);
        if (__ballot(on && !fin) != 0ull && lane == 0) col_flags[ci] = 1u;
        double cs = shift[ci];
        if (!has_shift[ci]) {
          const unsigned long long f = __ballot(on && fin);
          cs = 0.0;
          if (f) cs = __shfl(x, __builtin_ctzll(f), 64);
          if (lane == 0) {
            shift[ci] = cs;
            has_shift[ci] = f != 0ull;
          }
        }
        dv = on && fin ? x - cs : 0.0;
        m = __ballot(on);
      }
      Dt[ci * kCmStride + lane] = dv;
      if (lane == 0) vm[ci] = m;
    }
    __syncthreads();
    if (chunk + 1 < chunk1) load_chunk(chunk + 1);
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      if (s_ti[s] < 0) continue;  // (wave-uniform)
      const double* pa = Dt + (s_ti[s] * 16 + li) * kCmStride + lk;
      if constexpr (MASKED) {
        const double* pb = Dt + (s_tj[s] * 16 + li) * kCmStride + lk;
        const unsigned long long ma = vm[s_ti[s] * 16 + li] >> lk, mb = vm[s_tj[s] * 16 + li] >> lk;
#pragma unroll 4
        for (int t = 0; t < kCmSteps; ++t) {
          const double a = pa[4 * t], b = pb[4 * t];
          const double va = (double)(uint32_t)((ma >> (4 * t)) & 1ull), vb = (double)(uint32_t)((mb >> (4 * t)) & 1ull);
          acc[s][0] = cm_mfma(a, b, acc[s][0]);       // Sxy
          acc[s][1] = cm_mfma(a, vb, acc[s][1]);      // Sx
          acc[s][2] = cm_mfma(va, b, acc[s][2]);      // Sy
          acc[s][3] = cm_mfma(a * a, vb, acc[s][3]);  // Sxx
          acc[s][4] = cm_mfma(va, b * b, acc[s][4]);  // Syy
          acc[s][5] = cm_mfma(va, vb, acc[s][5]);     // n
        }
      } else if (s_tj[s] == T) {
#pragma unroll 4
        for (int t = 0; t < kCmSteps; ++t)
          acc[s][0] = cm_mfma(pa[4 * t], r0 + 4 * t + lk < end_row ? 1.0 : 0.0, acc[s][0]);
      } else {
        const double* pb = Dt + (s_tj[s] * 16 + li) * kCmStride + lk;
#pragma unroll 4
        for (int t = 0; t < kCmSteps; ++t) acc[s][0] = cm_mfma(pa[4 * t], pb[4 * t], acc[s][0]);
      }
    }
    if (!slab_end) continue;  // (uniform over the workgroup)

    // ---- the slab's sums -> states, folded into this range's running states
    const int64_t row0 = slab * kCorrmatSlabRows, row1 = corrmat_slab_end(slab, n_slabs, n_rows);
    if (!MASKED) {  // Σ d_i from the ones tiles, Σ d_i² from the diagonals
#pragma unroll
      for (int s = 0; s < kSlots; ++s) {
        if (s_ti[s] < 0) continue;
        if (s_tj[s] == T) {
          if (li == 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) col_sum[s_ti[s] * 16 + lk + 4 * g] = acc[s][0][g];
          }
        } else if (s_tj[s] == s_ti[s] && li >= lk && ((li - lk) & 3) == 0) {
          col_sq[s_ti[s] * 16 + li] = cm_pick(acc[s][0], (li - lk) >> 2);
        }
      }
      __syncthreads();
    }
    const bool first = slab == slab0;
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      if (s_ti[s] < 0 || s_tj[s] == T) continue;
      const int gj = s_tj[s] * 16 + li;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int gi = s_ti[s] * 16 + lk + 4 * g;
        if (gi > gj || gj >= k) continue;
        const int64_t p = corrmat_pair_index(gi, gj, k);
        double n, s_x, s_y, s_xx, s_yy, s_xy;
        if constexpr (MASKED) {
          s_xy = acc[s][0][g];
          s_x = acc[s][1][g];
          s_y = acc[s][2][g];
          s_xx = acc[s][3][g];
          s_yy = acc[s][4][g];
          n = acc[s][5][g];
        } else {
          n = (double)(row1 - row0);
          s_xy = acc[s][0][g];
          s_x = col_sum[gi];
          s_y = col_sum[gj];
          s_xx = col_sq[gi];
          s_yy = col_sq[gj];
        }
        CorrAcc run;
        if (first) run.n = run.xavg = run.yavg = run.ck = run.xmk = run.ymk = 0.0;
        else run = my[p];
        const uint32_t why = corr_fold_slab(run, shift[gi], shift[gj], n, s_x, s_y, s_xx, s_yy, s_xy, gi == gj);
        if (why) atomicOr(&pair_flags[p], why);
        my[p] = run;
      }
    }
  }
}

// blockIdx.x = pair: dq_corr_reduce_kernel's fixed tree over the pair's range states, written (not
// merged) to batch[pair].
__global__ __launch_bounds__(kBlock) void dq_corrmat_reduce_kernel(const CorrAcc* __restrict__ partials, int n_ranges,
                                                                   int64_t n_pairs, CorrAcc* __restrict__ batch) {
  __shared__ CorrAcc slot[kBlock];
  const int per = (n_ranges + kBlock - 1) / kBlock;
  const int b0 = threadIdx.x * per;
  CorrAcc a;
  a.n = a.xavg = a.yavg = a.ck = a.xmk = a.ymk = 0.0;
  for (int b = b0; b < b0 + per && b < n_ranges; ++b) corr_merge(a, partials[(int64_t)b * n_pairs + blockIdx.x]);
  slot[threadIdx.x] = a;
  __syncthreads();
  for (int s = 1; s < kBlock; s <<= 1) {
    if ((threadIdx.x % (2 * s)) == 0) corr_merge(slot[threadIdx.x], slot[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) batch[blockIdx.x] = slot[0];
}

// The pairs whose sums of finite values were not finite (kCorrmatNonFinite), by Spark's per-row update
// (corr_update_row): blockIdx.y = task {x, y, where}, blockIdx.x = contiguous row range, a lane takes
// every kBlock-th row of the range; lanes, waves and blocks merge in a fixed order.  One state per
// block at partials[range][task], for dq_corrmat_reduce_kernel.
__global__ __launch_bounds__(kBlock) void dq_corrmat_rows_kernel(const CorrTask* __restrict__ tasks,
                                                                 const DevColumn* __restrict__ cols,
                                                                 const DevMask* __restrict__ masks, int64_t n_rows,
                                                                 CorrAcc* __restrict__ partials) {
  const CorrTask task = tasks[blockIdx.y];
  const DevColumn& X = cols[task.x];
  const DevColumn& Y = cols[task.y];
  const uint64_t* wt = task.where_mask >= 0 ? masks[task.where_mask].t : nullptr;
  const int64_t per_block = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per_block;
  const int64_t r1 = r0 + per_block < n_rows ? r0 + per_block : n_rows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CorrAcc a;
  a.n = a.xavg = a.yavg = a.ck = a.xmk = a.ymk = 0.0;
  for (int64_t row = r0 + threadIdx.x; row < r1; row += kBlock) {
    if ((X.validity && !((X.validity[row >> 3] >> (row & 7)) & 1u)) ||
        (Y.validity && !((Y.validity[row >> 3] >> (row & 7)) & 1u)) || (wt && !((wt[row >> 6] >> (row & 63)) & 1ull)))
      continue;
    corr_update_row(a, cm_to_double(X.type, cm_load_raw(X, row)), cm_to_double(Y.type, cm_load_raw(Y, row)));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    CorrAcc o;
    o.n = __shfl_down(a.n, d, 64);
    o.xavg = __shfl_down(a.xavg, d, 64);
    o.yavg = __shfl_down(a.yavg, d, 64);
    o.ck = __shfl_down(a.ck, d, 64);
    o.xmk = __shfl_down(a.xmk, d, 64);
    o.ymk = __shfl_down(a.ymk, d, 64);
    if (lane < d) corr_merge(a, o);
  }
  __shared__ CorrAcc part[kBlock / 64];
  if (lane == 0) part[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    CorrAcc r = part[0];
    for (int w = 1; w < kBlock / 64; ++w) corr_merge(r, part[w]);
    partials[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = r;
  }
}

// running[p] += the batch's state of pair p: the pair kernel's (fallback[fb_index[p]]) where
// fb_index[p] >= 0, else the matrix's (batch[p]).  fb_index may be nullptr: no pair fell back.
__global__ __launch_bounds__(kBlock) void dq_corrmat_combine_kernel(const CorrAcc* __restrict__ batch,
                                                                    const CorrAcc* __restrict__ fallback,
                                                                    const int32_t* __restrict__ fb_index, int64_t n_pairs,
                                                                    CorrAcc* __restrict__ running) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n_pairs) return;
  const int32_t f = fb_index ? fb_index[p] : -1;
  CorrAcc run = running[p];
  corr_merge(run, f >= 0 ? fallback[f] : batch[p]);
  running[p] = run;
}

hipError_t launch_corrmat(bool masked, const DevColumn* d_cols, const int32_t* d_sel, int k, const uint64_t* d_where_t,
                          int64_t n_rows, int64_t slabs_per_range, int n_ranges, CorrAcc* d_partials, CorrAcc* d_batch,
                          uint32_t* d_pair_flags, uint32_t* d_col_flags, hipStream_t stream) {
  if (k <= 0 || k > kCorrmatMaxCols || n_rows <= 0 || n_ranges <= 0) return hipErrorInvalidValue;
  if (masked)
    hipLaunchKernelGGL(dq_corrmat_kernel<true>, dim3(n_ranges), dim3(kBlock), 0, stream, d_cols, d_sel, k, d_where_t,
                       n_rows, slabs_per_range, d_partials, d_pair_flags, d_col_flags);
  else
    hipLaunchKernelGGL(dq_corrmat_kernel<false>, dim3(n_ranges), dim3(kBlock), 0, stream, d_cols, d_sel, k, d_where_t,
                       n_rows, slabs_per_range, d_partials, d_pair_flags, d_col_flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_corrmat_reduce_kernel, dim3((unsigned)corrmat_pairs(k)), dim3(kBlock), 0, stream, d_partials,
                     n_ranges, corrmat_pairs(k), d_batch);
  return hipGetLastError();
}

hipError_t launch_corrmat_rows(const CorrTask* d_tasks, int n_tasks, const DevColumn* d_cols, const DevMask* d_masks,
                               int64_t n_rows, int blocks_per_task, CorrAcc* d_partials, CorrAcc* d_out, hipStream_t stream) {
  if (n_tasks <= 0 || n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_corrmat_rows_kernel, dim3(blocks_per_task, n_tasks), dim3(kBlock), 0, stream, d_tasks, d_cols,
                     d_masks, n_rows, d_partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_corrmat_reduce_kernel, dim3(n_tasks), dim3(kBlock), 0, stream, d_partials, blocks_per_task,
                     (int64_t)n_tasks, d_out);
  return hipGetLastError();
}

hipError_t launch_corrmat_combine(const CorrAcc* d_batch, const CorrAcc* d_fallback, const int32_t* d_fb_index,
                                  int64_t n_pairs, CorrAcc* d_running, hipStream_t stream) {
  if (n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_corrmat_combine_kernel, dim3((unsigned)((n_pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                     d_batch, d_fallback, d_fb_index, n_pairs, d_running);
  return hipGetLastError();
}

}  // namespace dq
