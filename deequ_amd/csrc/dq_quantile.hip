// dq_quantile.hip -- ApproxQuantile's batch summary on gfx950: the values at all target ranks of all
// (column, relativeError) pairs of a run by one MSD radix select over the 64-bit sortable key
// (dq_quantile.h), without sorting the column.
//
// A pass is two launches, blockIdx.y = pair, with no host round trip in between:
//
// dq_aq_count_kernel reads the column once (non-temporal loads, validity bitmap and Arrow offset as
// the KLL kernels read them).  The active prefixes -- the key prefixes that still hold a target rank,
// at most as many as target ranks -- sit sorted in LDS; a row finds its prefix by a branch-free
// binary search and counts into the workgroup's LDS counter of (prefix, next digit).  The digit is
// as wide as the 32768 LDS counters allow for the pass's number of prefixes (dq_aq::digit_bits):
// 15 bits for the first pass, 7 for up to 256 prefixes (relativeError 0.01: 8 passes in all), 4 for
// up to 2048 (relativeError 0.001: 14 passes).  So counting is always privatised in LDS; before the
// LDS atomic, two rounds of wave aggregation fold the lanes that share the first remaining lane's
// counter into one add, which is what a constant or two-valued column sends every row to.  The
// workgroup then adds its non-zero counters to the pair's global ones.
//
// dq_aq_plan_kernel (one workgroup per pair) prefix-sums the counters, places every target rank in
// its digit, and emits the next pass's sorted prefixes with the rows before each and its first
// target rank; after the first pass it also fixes n, gap and the number of ranks.  When all 64 bits
// are consumed a prefix is a key: the key of every target rank is written out.
#include <algorithm>

#include "dq_internal.h"
#include "dq_quantile.h"

namespace dq {

namespace {

using namespace aq;

// The tile's rows of this thread as doubles.  Every load is issued before any is used (a row past the
// end reads the last row again and a NULL row's slot is read like any other: both are dropped by
// the caller), so a thread has kRowsPerThread loads in flight instead of one.
template <typename T>
__device__ inline void load_rows(const void* v, int64_t r0, int64_t last, double (&out)[kRowsPerThread]) {
  const T* p = static_cast<const T*>(v);
  T raw[kRowsPerThread];
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) {
    const int64_t row = r0 + (int64_t)q * kSelectBlock + threadIdx.x;
    raw[q] = __builtin_nontemporal_load(p + (row < last ? row : last));
  }
#pragma unroll
  for (int q = 0; q < kRowsPerThread; ++q) out[q] = (double)raw[q];  // (int64: to nearest even, as Long.toDouble)
}

// number of target ranks <= x (0 <= x <= n < 2^31)
__device__ inline int64_t ranks_upto(int64_t x, int64_t n, int64_t gap, int64_t m) {
  if (x < 1) return 0;
  if (x >= n) return m;
  const int64_t c = (int64_t)((uint32_t)(x - 1) / (uint32_t)gap) + 1;
  return c < m - 1 ? c : m - 1;
}

// Exclusive scan of one value per thread over the workgroup; *total = the sum.  `scratch` holds one
// word per wave.  Ends with a barrier; the caller may reuse scratch after it.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* scratch, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  __syncthreads();
  if (lane == 63) scratch[wave] = incl;
  __syncthreads();
  uint32_t before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kSelectBlock / 64; ++w) {
    const uint32_t c = scratch[w];
    if (w < wave) before += c;
    sum += c;
  }
  *total = sum;
  __syncthreads();
  return before + incl - v;
}

}  // namespace

__global__ __launch_bounds__(kSelectBlock) void dq_aq_count_kernel(const DevAqPair* __restrict__ pairs,
                                                                   DevAqWork* __restrict__ work, int64_t n_rows,
                                                                   int pass) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds);                       // kCounters
  uint64_t* act = reinterpret_cast<uint64_t*>(lds + (size_t)kCounters * 4);  // kMaxRanks
  const DevAqPair& pair = pairs[blockIdx.y];
  DevAqWork& W = work[blockIdx.y];
  int n_active = 1, consumed = 0, bits = kCountersLog, cur = 0;
  if (pass > 0) {
    if (W.st.done) return;
    n_active = W.st.n_active;
    consumed = W.st.consumed;
    bits = W.st.bits;
    cur = W.st.cur;
  }
  if (n_active < 1 || n_active > kMaxRanks || bits < 1 || consumed + bits > 64 || (n_active << bits) > kCounters) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n_bins = n_active << bits;
  int np = 1;
  while (np < n_active) np <<= 1;
  for (int i = tid; i < n_bins; i += kSelectBlock) hist[i] = 0;
  for (int i = tid; i < np; i += kSelectBlock) act[i] = i < n_active ? W.prefix[cur][i] : ~0ull;
  __syncthreads();

  const int type = pair.type;
  const uint8_t* vbits = pair.validity;
  const int64_t bo = pair.bit_offset;
  const int digit_shift = 64 - consumed - bits;
  const uint32_t digit_mask = (1u << bits) - 1u;
  constexpr int64_t kTile = (int64_t)kSelectBlock * kRowsPerThread;

  for (int64_t r0 = (int64_t)blockIdx.x * kTile; r0 < n_rows; r0 += (int64_t)gridDim.x * kTile) {
    double val[kRowsPerThread];
    uint32_t vbyte[kRowsPerThread];
    if (vbits) {
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) {
        const int64_t row = r0 + (int64_t)q * kSelectBlock + tid;
        vbyte[q] = vbits[(bo + (row < n_rows ? row : n_rows - 1)) >> 3];
      }
    } else {
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) vbyte[q] = 1u;
    }
    switch (type) {
      case DQ_T_INT8: load_rows<int8_t>(pair.values, r0, n_rows - 1, val); break;
      case DQ_T_INT16: load_rows<int16_t>(pair.values, r0, n_rows - 1, val); break;
      case DQ_T_INT32: load_rows<int32_t>(pair.values, r0, n_rows - 1, val); break;
      case DQ_T_INT64: load_rows<int64_t>(pair.values, r0, n_rows - 1, val); break;
      case DQ_T_FLOAT32: load_rows<float>(pair.values, r0, n_rows - 1, val); break;
      default: load_rows<double>(pair.values, r0, n_rows - 1, val); break;
    }
    if (vbits) {
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) vbyte[q] >>= (uint32_t)((bo + r0 + (int64_t)q * kSelectBlock + tid) & 7);
    }
    uint64_t key[kRowsPerThread], p[kRowsPerThread];
    int idx[kRowsPerThread];
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      key[q] = key_of_bits(canonical_bits((uint64_t)__double_as_longlong(val[q])));
      p[q] = consumed ? key[q] >> (64 - consumed) : 0ull;
      idx[q] = 0;
    }
    for (int step = np >> 1; step > 0; step >>= 1) {  // the rows' searches side by side
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q)
        if (act[idx[q] + step] <= p[q]) idx[q] += step;
    }
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      const int64_t row = r0 + (int64_t)q * kSelectBlock + tid;
      const bool counts = row < n_rows && (vbyte[q] & 1u) && act[idx[q]] == p[q];
      const uint32_t bin = ((uint32_t)idx[q] << bits) | ((uint32_t)(key[q] >> digit_shift) & digit_mask);
      // lanes that share the first remaining lane's counter become one add (two rounds)
      uint64_t rem = __ballot(counts);
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        if (rem == 0) break;
        const int leader = __ffsll((unsigned long long)rem) - 1;
        const uint32_t lb = __shfl(bin, leader, 64);
        const uint64_t same = __ballot(counts && bin == lb) & rem;
        if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
        rem &= ~same;
      }
      if ((rem >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < n_bins; i += kSelectBlock) {
    const uint32_t c = hist[i];
    if (c) atomicAdd(&W.hist[i], c);
  }
}

__global__ __launch_bounds__(kSelectBlock) void dq_aq_plan_kernel(const DevAqPair* __restrict__ pairs,
                                                                  DevAqWork* __restrict__ work, int pass) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds);                         // kCounters: counts, then their scan
  uint32_t* scratch = reinterpret_cast<uint32_t*>(lds + (size_t)kCounters * 4);  // one word per wave
  uint32_t* base = scratch + kSelectBlock / 64;                                  // kMaxRanks: rows before each prefix
  const DevAqPair& pair = pairs[blockIdx.y];
  DevAqWork& W = work[blockIdx.y];
  int n_active = 1, consumed = 0, bits = kCountersLog, cur = 0;
  if (pass > 0) {
    if (W.st.done) return;
    n_active = W.st.n_active;
    consumed = W.st.consumed;
    bits = W.st.bits;
    cur = W.st.cur;
  }
  if (n_active < 1 || n_active > kMaxRanks || bits < 1 || consumed + bits > 64 || (n_active << bits) > kCounters) {
    if (threadIdx.x == 0) {
      W.st.error = 1;
      W.st.done = 1;
    }
    return;
  }
  const int tid = threadIdx.x;
  const int n_bins = n_active << bits;
  constexpr int kPer = kCounters / kSelectBlock;  // consecutive counters per thread
  const int i0 = tid * kPer;

  for (int i = tid; i < n_active; i += kSelectBlock) base[i] = W.base[cur][i];
  // counts -> LDS, the global counters zeroed for the next pass
  // (counters at and past n_bins are never written and stay zero, so the whole array is read and cleared)
  uint32_t cnt[kPer];
  uint32_t mine = 0;
  uint4* gh = reinterpret_cast<uint4*>(W.hist + i0);
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) {
    const uint4 v = gh[k];
    cnt[4 * k] = v.x;
    cnt[4 * k + 1] = v.y;
    cnt[4 * k + 2] = v.z;
    cnt[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < kPer / 4; ++k) gh[k] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int k = 0; k < kPer; ++k) mine += cnt[k];
  uint32_t total = 0;
  uint32_t run = block_scan(mine, scratch, &total);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    hist[i0 + k] = run;  // exclusive scan over all counters
    run += cnt[k];
  }
  __syncthreads();

  int64_t n, gap, m;
  if (pass == 0) {
    n = (int64_t)total;  // the one (empty) prefix holds every valid row
    gap = n > 0 ? batch_gap(pair.eps, n) : 1;
    m = n > 0 ? batch_ranks(n, gap) : 0;
    if (tid == 0) {
      W.st.n = n;
      W.st.gap = gap;
      W.st.m = m;
    }
    if (n == 0 || m > kMaxRanks) {
      if (tid == 0) {
        W.st.error = m > kMaxRanks ? 1 : 0;
        W.st.done = 1;
      }
      return;
    }
  } else {
    n = W.st.n;
    gap = W.st.gap;
    m = W.st.m;
  }

  // the (prefix, digit) pairs that hold a target rank, in order
  auto child = [&](int k, uint32_t* before_out, uint32_t* jlo_out) -> bool {
    const int i = i0 + k;
    if (i >= n_bins || !cnt[k]) return false;
    const int a = i >> bits;
    const int64_t before = (int64_t)base[a] + (int64_t)(hist[i] - hist[a << bits]);
    const int64_t lo = ranks_upto(before, n, gap, m), hi = ranks_upto(before + cnt[k], n, gap, m);
    *before_out = (uint32_t)before;
    *jlo_out = (uint32_t)lo;
    return hi > lo;
  };
  uint32_t flags = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    uint32_t b, j;
    if (child(k, &b, &j)) flags |= 1u << k;
  }
  uint32_t n_next = 0;
  uint32_t at = block_scan((uint32_t)__popc(flags), scratch, &n_next);
  if (n_next < 1 || n_next > (uint32_t)kMaxRanks) {  // (cannot happen: every child holds a rank of its own)
    if (tid == 0) {
      W.st.error = 1;
      W.st.done = 1;
    }
    return;
  }
  const int nxt = cur ^ 1;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (flags & (1u << k)) {
      const int i = i0 + k, a = i >> bits;
      uint32_t b = 0, j = 0;
      child(k, &b, &j);
      W.prefix[nxt][at] = (W.prefix[cur][a] << bits) | (uint64_t)(i & ((1 << bits) - 1));
      W.base[nxt][at] = b;
      W.jlo[nxt][at] = j;
      ++at;
    }
  }
  const int now = consumed + bits;
  __threadfence();
  __syncthreads();
  if (now == 64) {  // a prefix is a key: rank j belongs to the last prefix with jlo <= j
    int np = 1;
    while (np < (int)n_next) np <<= 1;
    for (int64_t j = tid; j < m; j += kSelectBlock) {
      int idx = 0;
      for (int step = np >> 1; step > 0; step >>= 1)
        if (idx + step < (int)n_next && (int64_t)W.jlo[nxt][idx + step] <= j) idx += step;
      W.keys[j] = W.prefix[nxt][idx];
    }
  }
  if (tid == 0) {
    W.st.n_active = (int32_t)n_next;
    W.st.consumed = now;
    W.st.bits = now < 64 ? digit_bits((int)n_next, now) : 0;
    W.st.cur = nxt;
    W.st.done = now == 64 ? 1 : 0;
  }
}

static hipError_t allow_lds(const void* fn, uint32_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

// One pass over the batch for every pair: count, then plan.
hipError_t launch_aq_pass(const aq::DevAqPair* d_pairs, aq::DevAqWork* d_work, int n_pairs, int64_t n_rows, int pass,
                          hipStream_t stream) {
  if (n_pairs <= 0) return hipSuccess;
  const uint32_t count_lds = (uint32_t)((size_t)kCounters * 4 + (size_t)kMaxRanks * 8);
  const uint32_t plan_lds = (uint32_t)((size_t)kCounters * 4 + (size_t)(kSelectBlock / 64) * 4 + (size_t)kMaxRanks * 4);
  hipError_t e = allow_lds(reinterpret_cast<const void*>(dq_aq_count_kernel), count_lds);
  if (e != hipSuccess) return e;
  e = allow_lds(reinterpret_cast<const void*>(dq_aq_plan_kernel), plan_lds);
  if (e != hipSuccess) return e;
  constexpr int64_t kTile = (int64_t)kSelectBlock * kRowsPerThread;
  const int64_t tiles = (n_rows + kTile - 1) / kTile;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, kMaxBlocksPerPair));
  if (n_rows > 0)
    hipLaunchKernelGGL(dq_aq_count_kernel, dim3(blocks, n_pairs), dim3(kSelectBlock), count_lds, stream, d_pairs, d_work,
                       n_rows, pass);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_aq_plan_kernel, dim3(1, n_pairs), dim3(kSelectBlock), plan_lds, stream, d_pairs, d_work, pass);
  return hipGetLastError();
}

}  // namespace dq
