// dq_kll.hip -- KLLSketch on gfx950: the reference's sequential sketch (QuantileNonSample.scala,
// NonSampleCompactor.scala) reproduced item for item on a fixed partitioning (dq_kll.h).
//
// dq_kll_slab_kernel: one workgroup per (slab, column); blockIdx.y is the column, so every KLL column
// of a run goes in one launch per batch.  The workgroup keeps all levels of its sketch in LDS and
// emulates `update` in bulk: with room = total - actual it appends the next room + 1 non-NULL items
// to level 0 in row order (a block prefix sum over the validity bits; slab starts need no alignment),
// which is exactly where the reference's `actual > total` trigger fires, then runs one `condense`:
// an LDS bitonic sort of the lowest level at or over its capacity, alternate elements appended to
// the level above, the odd tail (the last appended item) kept.  All control flow is workgroup-uniform.
//
// dq_kll_merge_kernel: one round of the balanced tree: slab 2 step j absorbs slab 2 step j + step
// with the reference's `merge` (buffers concatenated level by level, `this` keeps numOfCompress and
// offset, condense while actual >= total).  Both sketches' items are resident in LDS at once.
//
// LDS layout: the levels are stacked top level first, level 0 last, so the hot append grows the
// pool's end and a compaction's output lands exactly where the level above ends; the levels below a
// compacted level > 0 slide down by the items that left.  Items are sortable uint64 keys (dq_kll.h).
#include "dq_internal.h"
#include "dq_kll.h"

namespace dq {

namespace {

using namespace kll;

constexpr int kRowsPerThread = 4;
constexpr int kChunkRows = kRowsPerThread * kBlock;
constexpr int kWaves = kBlock / 64;

struct KllLds {
  int32_t len[kMaxLevels], nc[kMaxLevels], off[kMaxLevels], cap[kMaxLevels];
  int32_t n_levels, actual, total, error;
  int32_t has_nan, pad;
  unsigned long long min_key, max_key;
  long long next_row;
  uint32_t wave_cnt[kWaves];
};
static_assert(sizeof(KllLds) <= (size_t)kLdsReserveBytes, "the level tables must fit the reserved LDS");

__device__ inline void cmpx(uint64_t* a, int lo, int hi) {
  const uint64_t x = a[lo], y = a[hi];
  if (key_ord(y) < key_ord(x)) {
    a[lo] = y;
    a[hi] = x;
  }
}

// Ascending bitonic network over a[0 .. n) for any n: every comparator puts the smaller key at the
// lower index (the first step of a merge stage mirrors), so the slots at and past n act as +infinity
// and their comparators are skipped.  Called by the whole workgroup after a barrier; ends with one.
__device__ void lds_sort(uint64_t* a, int n) {
  if (n < 2) return;
  int np = 2;
  while (np < n) np <<= 1;
  const int half = np >> 1;
  for (int k = 2, lk = 1; k <= np; k <<= 1, ++lk) {
    const int hk = k >> 1;
    for (int t = threadIdx.x; t < half; t += kBlock) {
      const int blk = t >> (lk - 1), i = t & (hk - 1);
      const int lo = blk * k + i, hi = blk * k + k - 1 - i;
      if (hi < n) cmpx(a, lo, hi);
    }
    __syncthreads();
    for (int j = hk >> 1; j >= 1; j >>= 1) {
      for (int t = threadIdx.x; t < half; t += kBlock) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
        if (hi < n) cmpx(a, lo, hi);
      }
      __syncthreads();
    }
  }
}

// QuantileNonSample.condense: one compaction at the lowest level at or over its capacity.
__device__ void condense(KllLds& S, uint64_t* pool) {
  const int H = S.n_levels;
  int h = 0;
  while (h < H && S.len[h] < S.cap[h]) ++h;
  const bool grow = h + 1 >= H;
  int s = 0, end = 0;
  for (int g = H - 1; g >= 0; --g) {
    if (g > h) s += S.len[g];
    end += S.len[g];
  }
  const int L = h < H ? S.len[h] : 0, Le = L & ~1, m = Le >> 1;
  int off = h < H ? S.off[h] : 0;
  if (h < H && (S.nc[h] & 1)) off = 1 - off;
  __syncthreads();
  if (h == H || (grow && H >= kMaxLevels)) {  // (no level at capacity cannot happen: actual >= total)
    if (threadIdx.x == 0) S.error = 2;
    __syncthreads();
    return;
  }
  lds_sort(pool + s, Le);
  for (int base = 0; base < m; base += kBlock) {  // sorted[off], sorted[off + 2], ... -> the level above
    const int i = base + threadIdx.x;
    uint64_t v = 0;
    if (i < m) v = pool[s + off + 2 * i];
    __syncthreads();
    if (i < m) pool[s + i] = v;
  }
  const int src = s + Le, cnt = end - src;  // the odd tail and every lower level slide down by m
  for (int base = 0; base < cnt; base += kBlock) {
    const int i = base + threadIdx.x;
    uint64_t v = 0;
    if (i < cnt) v = pool[src + i];
    __syncthreads();
    if (i < cnt) pool[s + m + i] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (grow) {
      S.n_levels = H + 1;
      S.len[H] = 0;
      S.nc[H] = 0;
      S.off[H] = 0;
      S.total += S.cap[H];
    }
    S.len[h + 1] += m;
    S.len[h] = L & 1;
    S.off[h] = off;
    S.nc[h] += 1;
    S.actual = end - m;
  }
  __syncthreads();
}

__device__ inline double load_value(const void* v, int type, int64_t row) {
  switch (type) {
    case DQ_T_INT8: return (double)static_cast<const int8_t*>(v)[row];
    case DQ_T_INT16: return (double)static_cast<const int16_t*>(v)[row];
    case DQ_T_INT32: return (double)static_cast<const int32_t*>(v)[row];
    case DQ_T_INT64: return (double)static_cast<const int64_t*>(v)[row];  // Long.toDouble: to nearest even
    case DQ_T_FLOAT32: return (double)static_cast<const float*>(v)[row];
    default: return static_cast<const double*>(v)[row];
  }
}

// The sketch in LDS -> its DevSketch and item block (level 0 first).
__device__ void store_sketch(const KllLds& S, const uint64_t* pool, DevSketch* out, uint64_t* items, int64_t stride) {
  const int err = S.error ? S.error : ((int64_t)S.actual > stride ? 1 : 0);
  const int H = err ? 0 : S.n_levels;
  if (threadIdx.x < kMaxLevels) {
    const int t = threadIdx.x;
    out->len[t] = t < H ? S.len[t] : 0;
    out->num_compress[t] = t < H ? S.nc[t] : 0;
    out->offset[t] = t < H ? S.off[t] : 0;
  }
  if (threadIdx.x == 0) {
    out->n_levels = err ? 1 : S.n_levels;
    out->error = err;
    out->has_nan = S.has_nan;
    out->pad = 0;
    out->min_key = S.min_key;
    out->max_key = S.max_key;
  }
  if (err) return;
  int above = S.actual, below = 0;
  for (int h = 0; h < H; ++h) {
    const int n = S.len[h];
    above -= n;  // the items of the levels over h come first in the pool
    for (int i = threadIdx.x; i < n; i += kBlock) items[below + i] = pool[above + i];
    below += n;
  }
}

}  // namespace

__global__ __launch_bounds__(kBlock) void dq_kll_slab_kernel(const DevKllColumn* __restrict__ cols, int64_t n_rows,
                                                             int64_t slab_rows, DevSketch* __restrict__ sketches,
                                                             uint64_t* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  KllLds& S = *reinterpret_cast<KllLds*>(lds);
  uint64_t* pool = reinterpret_cast<uint64_t*>(lds + kLdsReserveBytes);
  const DevKllColumn& col = cols[blockIdx.y];
  const int pool_items = col.pool_items;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kMaxLevels) {
    S.len[tid] = 0;
    S.nc[tid] = 0;
    S.off[tid] = 0;
    S.cap[tid] = col.cap[tid];
  }
  if (tid == 0) {
    S.n_levels = 1;
    S.actual = 0;
    S.total = col.cap[0];
    S.error = 0;
    S.has_nan = 0;
    S.min_key = key_of_bits((uint64_t)__double_as_longlong(kInitMin));
    S.max_key = key_of_bits((uint64_t)__double_as_longlong(kInitMax));
    S.next_row = 0;
  }
  __syncthreads();

  uint64_t tmin = S.min_key, tmax = S.max_key;
  bool tnan = false;
  int64_t r = (int64_t)blockIdx.x * slab_rows;
  const int64_t r_end = min(n_rows, r + slab_rows);
  const int type = col.type;
  const uint8_t* vbits = col.validity;
  const int64_t bo = col.bit_offset;

  while (r < r_end) {
    const int base = S.actual;
    const int want = S.total - base + 1;  // the update that makes actual > total
    if (want < 1 || base + want > pool_items) {
      __syncthreads();
      if (tid == 0) S.error = 1;
      break;
    }
    // this thread's rows of the chunk, in row order
    const int64_t row0 = r + (int64_t)tid * kRowsPerThread;
    uint64_t key[kRowsPerThread];
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      const int64_t row = row0 + q;
      key[q] = 0;
      if (row < r_end) {
        const int64_t b = bo + row;
        if (!vbits || ((vbits[b >> 3] >> (b & 7)) & 1u)) {
          mask |= 1u << q;
          key[q] = key_of_bits((uint64_t)__double_as_longlong(load_value(col.values, type, row)));
        }
      }
    }
    const uint32_t cnt = __popc(mask);
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) S.wave_cnt[wave] = incl;
    __syncthreads();
    uint32_t before = 0, chunk_total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const uint32_t c = S.wave_cnt[w];
      if (w < wave) before += c;
      chunk_total += c;
    }
    uint32_t idx = before + incl - cnt;
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      if (mask & (1u << q)) {
        if (idx < (uint32_t)want) {
          const uint64_t k = key[q];
          pool[base + idx] = k;
          if (key_is_nan(k)) {
            tnan = true;
          } else {
            tmin = k < tmin ? k : tmin;
            tmax = k > tmax ? k : tmax;
          }
          if (idx == (uint32_t)want - 1) S.next_row = row0 + q + 1;
        }
        ++idx;
      }
    }
    const int take = chunk_total < (uint32_t)want ? (int)chunk_total : want;
    __syncthreads();
    r = chunk_total > (uint32_t)want ? (int64_t)S.next_row : min(r + (int64_t)kChunkRows, r_end);
    if (tid == 0) {
      S.actual = base + take;
      S.len[0] += take;
    }
    __syncthreads();
    if (take == want) {
      condense(S, pool);
      if (S.error) break;
    }
  }
  __syncthreads();
  if (tnan) S.has_nan = 1;
  atomicMin(&S.min_key, (unsigned long long)tmin);
  atomicMax(&S.max_key, (unsigned long long)tmax);
  __syncthreads();
  const int64_t slot = col.sketch_base + blockIdx.x;
  store_sketch(S, pool, sketches + slot, items + col.item_base + (int64_t)blockIdx.x * col.stride, col.stride);
}

__global__ __launch_bounds__(kBlock) void dq_kll_merge_kernel(const DevKllColumn* __restrict__ cols, int64_t n_slabs,
                                                              int64_t step, int pool_items,
                                                              DevSketch* __restrict__ sketches,
                                                              uint64_t* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  KllLds& S = *reinterpret_cast<KllLds*>(lds);
  uint64_t* pool = reinterpret_cast<uint64_t*>(lds + kLdsReserveBytes);
  const DevKllColumn& col = cols[blockIdx.y];
  const int64_t a = 2 * step * (int64_t)blockIdx.x, b = a + step;
  if (b >= n_slabs) return;
  DevSketch* A = sketches + col.sketch_base + a;
  const DevSketch* B = sketches + col.sketch_base + b;
  uint64_t* ia = items + col.item_base + a * col.stride;
  const uint64_t* ib = items + col.item_base + b * col.stride;
  const int tid = threadIdx.x;
  const int HA = min(max(A->n_levels, 1), kMaxLevels), HB = min(max(B->n_levels, 1), kMaxLevels);
  const int H = max(HA, HB);
  if (tid < kMaxLevels) {
    const int la = tid < HA ? A->len[tid] : 0, lb = tid < HB ? B->len[tid] : 0;
    S.len[tid] = la + lb;
    S.nc[tid] = tid < HA ? A->num_compress[tid] : 0;  // `this` keeps its own numOfCompress / offset
    S.off[tid] = tid < HA ? A->offset[tid] : 0;
    S.cap[tid] = col.cap[tid];
  }
  __syncthreads();
  if (tid == 0) {
    int actual = 0, total = 0;
    for (int h = 0; h < H; ++h) {
      actual += S.len[h];
      total += S.cap[h];
    }
    S.n_levels = H;
    S.actual = actual;
    S.total = total;
    S.error = A->error | B->error;
    if (!S.error && actual > pool_items) S.error = 1;
    S.has_nan = A->has_nan | B->has_nan;
    S.min_key = A->min_key < B->min_key ? A->min_key : B->min_key;
    S.max_key = A->max_key > B->max_key ? A->max_key : B->max_key;
  }
  __syncthreads();
  if (!S.error) {
    int above = S.actual, oa = 0, ob = 0;
    for (int h = 0; h < H; ++h) {
      const int la = h < HA ? A->len[h] : 0, lb = h < HB ? B->len[h] : 0;
      above -= la + lb;
      for (int i = tid; i < la; i += kBlock) pool[above + i] = ia[oa + i];
      for (int i = tid; i < lb; i += kBlock) pool[above + la + i] = ib[ob + i];
      oa += la;
      ob += lb;
    }
    __syncthreads();
    while (S.actual >= S.total && !S.error) condense(S, pool);
  }
  __syncthreads();
  store_sketch(S, pool, A, ia, col.stride);
}

static hipError_t allow_lds(const void* fn, uint32_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

hipError_t launch_kll_slabs(const kll::DevKllColumn* d_cols, int n_cols, int64_t n_rows, int64_t slab_rows,
                            int64_t n_slabs, uint32_t lds_bytes, kll::DevSketch* d_sketches, uint64_t* d_items,
                            hipStream_t stream) {
  if (n_cols <= 0 || n_slabs <= 0) return hipSuccess;
  hipError_t e = allow_lds(reinterpret_cast<const void*>(dq_kll_slab_kernel), lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_kll_slab_kernel, dim3((unsigned)n_slabs, n_cols), dim3(kBlock), lds_bytes, stream, d_cols,
                     n_rows, slab_rows, d_sketches, d_items);
  return hipGetLastError();
}

hipError_t launch_kll_merge(const kll::DevKllColumn* d_cols, int n_cols, int64_t n_slabs, int64_t step, int pool_items,
                            uint32_t lds_bytes, kll::DevSketch* d_sketches, uint64_t* d_items, hipStream_t stream) {
  const int64_t pairs = (n_slabs + 2 * step - 1) / (2 * step);
  if (n_cols <= 0 || pairs <= 0 || step >= n_slabs) return hipSuccess;
  hipError_t e = allow_lds(reinterpret_cast<const void*>(dq_kll_merge_kernel), lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_kll_merge_kernel, dim3((unsigned)pairs, n_cols), dim3(kBlock), lds_bytes, stream, d_cols,
                     n_slabs, step, pool_items, d_sketches, d_items);
  return hipGetLastError();
}

}  // namespace dq
