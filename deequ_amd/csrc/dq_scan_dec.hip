// dq_scan_dec.hip -- the fused scan of a decimal column (Arrow decimal128, Spark DecimalType(p, s))
// and the decimal -> double cast kernel.
//
// One pass over the column serves every scan-shareable analyzer on one (column, where): Size,
// Completeness, Sum, Mean, Minimum, Maximum, StandardDeviation and ApproxCountDistinct.  Each lane
// reads one row per load -- 16 bytes, one global_load_dwordx4, four loads in flight per lane -- with
// the row's validity bit and, when the task has a filter, its two mask bits.  Semantics per task
// (Spark 2.2.2; the state mapping is in dq_api.cpp):
//   sum, abs   : exact.  sum(decimal) is an exact decimal sum (Sum.scala:40 casts the result to
//                double once), so each row's four 32-bit limbs (the top one signed) go into four
//                64-bit lane accumulators -- a block's rows cannot overflow them -- and the block
//                recombines them into a 192-bit integer; no fp64 until dq_plan_finish.  Σ|x| rides
//                beside it: below 10^min(38, p + 10) no prefix in any order overflows Spark's
//                decimal(min(38, p + 10), s) buffer (SPARK-28067), at or above it the op is declined.
//   min, max   : signed 128-bit compares; converted once at finish.
//   mean, m2   : StatefulStdDevPop takes DoubleType, so every row is cast first (Decimal.toDouble =
//                BigDecimal.doubleValue, dq_decimal.h: the one-divide tier inline, the slower exact
//                tiers behind a wave-uniform branch) and fed to the shifted moments of the other
//                value scans (dq_scan_common.h), cancellation guard included.
//   HLL        : XxHash64Function.hash(v, DecimalType(p, s), 42) (InterpretedHashFunction):
//                precision <= 18 hashes the unscaled long (hashLong), precision > 18 the bytes of
//                BigInteger.toByteArray -- chosen by the column type, not the value -- into the
//                workgroup's LDS copy of the 512 registers (the hll_hash_update pattern).
// The partials are merged in a fixed order (one block per task), then folded into the plan's running
// accumulator in batch order: results are bitwise reproducible.
#include <algorithm>

#include "dq_scan_common.h"
#include "dq_strhash.h"
#include "dq_decimal.h"

namespace dq {

namespace {

using dec::u128;

constexpr int kDecUnroll = 4;  // 16-byte loads in flight per lane

__device__ inline bool less128(uint64_t alo, int64_t ahi, uint64_t blo, int64_t bhi) {
  return ahi < bhi || (ahi == bhi && alo < blo);
}

// a += b over 192 bits (two's complement)
__device__ inline void add192(uint64_t* a, const uint64_t* b) {
  const uint64_t r0 = a[0] + b[0];
  const uint64_t c0 = r0 < b[0] ? 1u : 0u;
  const uint64_t t1 = a[1] + b[1];
  const uint64_t c1a = t1 < b[1] ? 1u : 0u;
  const uint64_t r1 = t1 + c0;
  const uint64_t c1 = c1a + (r1 < c0 ? 1u : 0u);
  a[0] = r0;
  a[1] = r1;
  a[2] = a[2] + b[2] + c1;
}

// a += sext(v) << (32 j), j = 0..3 (`neg`: v is a negative int64)
__device__ inline void add_limb192(uint64_t* a, uint64_t v, bool neg, int j) {
  const uint64_t ext = neg ? ~0ull : 0ull;
  uint64_t b[3];
  switch (j) {
    case 0: b[0] = v; b[1] = ext; b[2] = ext; break;
    case 1: b[0] = v << 32; b[1] = (v >> 32) | (ext << 32); b[2] = ext; break;
    case 2: b[0] = 0; b[1] = v; b[2] = ext; break;
    default: b[0] = 0; b[1] = v << 32; b[2] = (v >> 32) | (ext << 32); break;
  }
  add192(a, b);
}

__device__ inline void dec_acc_init(DecAcc& a) {
  a.n_rows = a.n_wnn = a.n_sel = 0;
  a.sum[0] = a.sum[1] = a.sum[2] = 0;
  a.abs[0] = a.abs[1] = a.abs[2] = 0;
  a.min_lo = ~0ull;
  a.min_hi = INT64_MAX;
  a.max_lo = 0;
  a.max_hi = INT64_MIN;
  a.mean = a.m2 = 0.0;
}

// a <- a + b (b is the later partial), fixed operand order
__device__ inline void dec_acc_merge(DecAcc& a, const DecAcc& b) {
  double na = (double)a.n_sel;
  moments_merge(na, a.mean, a.m2, (double)b.n_sel, b.mean, b.m2);
  a.n_rows += b.n_rows;
  a.n_wnn += b.n_wnn;
  a.n_sel += b.n_sel;
  add192(a.sum, b.sum);
  add192(a.abs, b.abs);
  if (less128(b.min_lo, b.min_hi, a.min_lo, a.min_hi)) {
    a.min_lo = b.min_lo;
    a.min_hi = b.min_hi;
  }
  if (less128(a.max_lo, a.max_hi, b.max_lo, b.max_hi)) {
    a.max_lo = b.max_lo;
    a.max_hi = b.max_hi;
  }
}

// Cast of one row, the wave converged: the one-divide tier for every lane, the exact slow tiers only
// when a lane that counts (`need`) holds a value outside it.
__device__ inline double cast_row(uint64_t lo, int64_t hi, int scale, bool need) {
  const u128 mag = dec::magnitude(lo, hi);
  const bool fast = dec::tier_of(mag, scale) == 1;
  double x = dec::to_double_fast(mag, scale <= 22 ? scale : 0, hi < 0);
  if (__ballot(need && !fast)) {
    if (need && !fast) x = dec::to_double_slow(mag, scale, hi < 0);
  }
  return x;
}

// Spark's hash of one decimal of precision > 18, in the pre-final form hll_slot reads
__device__ inline W64 hash_bytes(uint64_t lo, int64_t hi) {
  const int len = dec::byte_length(lo, hi);
  const u128 st = dec::be_stream(lo, hi, len);
  const uint64_t s[3] = {(uint64_t)st, (uint64_t)(st >> 64), 0ull};
  return xxh64_words_dev(s, (uint32_t)len);
}

struct DecWavePart {
  uint64_t cnt[3];
  uint64_t s[4], a[4];
  uint64_t min_lo, max_lo;
  int64_t min_hi, max_hi;
  double n, mean, m2;
};

}  // namespace

__global__ __launch_bounds__(kBlock) void dq_scan_dec_kernel(const DecTask* __restrict__ tasks,
                                                             const DevColumn* __restrict__ cols,
                                                             const DevMask* __restrict__ masks, int64_t n_rows,
                                                             DecAcc* partials, uint32_t* __restrict__ hll_regs) {
  const DecTask& task = tasks[blockIdx.y];
  int64_t row_begin, row_end;
  chunk_of_block(n_rows, row_begin, row_end);
  __shared__ uint32_t lregs[kHllM];
  __shared__ DecWavePart part[kBlock / 64];
  const bool hll_on = (task.flags & DF_HLL) != 0;
  const bool stats_on = (task.flags & DF_STATS) != 0;
  const bool hash_long = task.precision <= 18;
  const int scale = task.scale;
  if (hll_on) {
    for (int r = threadIdx.x; r < kHllM; r += kBlock) lregs[r] = 0u;
    __syncthreads();
  }
  const DevColumn& col = cols[task.column];
  const dq_v4u* __restrict__ values = static_cast<const dq_v4u*>(col.values);
  const uint8_t* __restrict__ validity = col.validity;
  const bool has_where = task.where_mask >= 0;
  const uint64_t* __restrict__ wt_w = has_where ? masks[task.where_mask].t : nullptr;
  const uint64_t* __restrict__ wn_w = has_where ? masks[task.where_mask].nn : nullptr;

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  uint32_t n_rows_c = 0, n_wnn = 0, n_sel = 0;
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  uint64_t mn_lo = ~0ull, mx_lo = 0;
  int64_t mn_hi = INT64_MAX, mx_hi = INT64_MIN;
  double shift = 0.0, S1 = 0.0, S2 = 0.0;
  bool have_shift = false;  // wave-uniform

  // Every lane runs every iteration (rows past the chunk's end are clamped to its first row and
  // deselected), so the wave stays converged for the ballots below and no load sits behind a branch.
#pragma unroll 1
  for (int64_t base = row_begin; base < row_end; base += (int64_t)kBlock * kDecUnroll) {
    dq_v4u vec[kDecUnroll];
    uint32_t vbit[kDecUnroll], wt[kDecUnroll], wn[kDecUnroll];
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int64_t r = base + (int64_t)u * kBlock + tid;
      const bool in = r < row_end;
      const int64_t rc = in ? r : row_begin;
      vec[u] = values[rc];
      vbit[u] = validity ? (uint32_t)(validity[rc >> 3] >> (rc & 7)) & 1u : 1u;
      wt[u] = has_where ? (uint32_t)(wt_w[rc >> 6] >> (rc & 63)) & 1u : 1u;
      wn[u] = has_where ? (uint32_t)(wn_w[rc >> 6] >> (rc & 63)) & 1u : 1u;
      if (!in) vbit[u] = wt[u] = wn[u] = 0u;
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const uint32_t sel = vbit[u] & wt[u];
      n_rows_c += wt[u];
      n_wnn += wn[u];
      n_sel += sel;
      const uint64_t lo = (uint64_t)vec[u][0] | ((uint64_t)vec[u][1] << 32);
      const int64_t hi = (int64_t)((uint64_t)vec[u][2] | ((uint64_t)vec[u][3] << 32));
      if (stats_on) {
        const uint64_t m = sel ? ~0ull : 0ull;
        s0 += vec[u][0] & m;
        s1 += vec[u][1] & m;
        s2 += vec[u][2] & m;
        s3 += (uint64_t)(int64_t)(int32_t)vec[u][3] & m;
        const u128 mag = dec::magnitude(lo, hi);
        a0 += (uint32_t)mag & m;
        a1 += (uint32_t)(mag >> 32) & m;
        a2 += (uint32_t)(mag >> 64) & m;
        a3 += (uint32_t)(mag >> 96) & m;
        if (sel && less128(lo, hi, mn_lo, mn_hi)) {
          mn_lo = lo;
          mn_hi = hi;
        }
        if (sel && less128(mx_lo, mx_hi, lo, hi)) {
          mx_lo = lo;
          mx_hi = hi;
        }
        const double x = cast_row(lo, hi, scale, sel != 0u);
        if (!have_shift) {  // the wave's first selected value
          const uint64_t b = __ballot(sel != 0u);
          if (b) {
            shift = __shfl(x, __builtin_ctzll(b), 64);
            have_shift = true;
          }
        }
        const double d = sel ? (x - shift) : 0.0;
        S1 += d;
        S2 = fma(d, d, S2);
      }
      if (hll_on) {
        if (hash_long) {
          hll_hash_update<int64_t>(lregs, (int64_t)lo, sel);
        } else if (__ballot(sel != 0u)) {  // (a wave of NULL or filtered rows hashes nothing)
          uint32_t idx, nlz;
          hll_slot(hash_bytes(lo, hi), idx, nlz);
          __hip_atomic_fetch_max(&lregs[idx], (nlz + 1u) * sel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
  }
  if (hll_on) {  // fold the workgroup's registers into the task's set (max: order independent)
    __syncthreads();
    uint32_t* out = hll_regs + (int64_t)task.hll * kHllM;
    for (int r = threadIdx.x; r < kHllM; r += kBlock) {
      const uint32_t v = lregs[r];
      if (v) atomicMax(&out[r], v);
    }
  }
  // ---- moments per wave, with the cancellation guard of the shifted sums (dq_scan_common.h)
  uint64_t n_w = wave_sum_u64((uint64_t)n_sel);  // lane 0
  double W1 = wave_sum_f64(S1), W2 = wave_sum_f64(S2);
  if (stats_on) {  // (block-uniform)
    double wn_d = 0.0, wmean = 0.0;
    bool cancel = false;
    if (lane == 0 && n_w > 0) {
      wn_d = (double)n_w;
      wmean = shift + W1 / wn_d;
      cancel = moments_cancel(wn_d, W1, W2);
    }
    if (__syncthreads_or(cancel)) {
      // redo Σd, Σd² of the chunk about its mean; the lanes' selected counts move with them
      const double mblk = block_mean_of_waves(wn_d, wmean);
      shift = mblk;
      S1 = S2 = 0.0;
      n_sel = 0u;
#pragma unroll 1
      for (int64_t base = row_begin; base < row_end; base += kBlock) {
        const int64_t r = base + tid;
        const bool in = r < row_end;
        const int64_t rc = in ? r : row_begin;
        const dq_v4u v = values[rc];
        uint32_t sel = validity ? (uint32_t)(validity[rc >> 3] >> (rc & 7)) & 1u : 1u;
        if (has_where) sel &= (uint32_t)(wt_w[rc >> 6] >> (rc & 63)) & 1u;
        if (!in) sel = 0u;
        const uint64_t lo = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
        const int64_t hi = (int64_t)((uint64_t)v[2] | ((uint64_t)v[3] << 32));
        const double x = cast_row(lo, hi, scale, sel != 0u);
        const double d = sel ? (x - mblk) : 0.0;
        S1 += d;
        S2 = fma(d, d, S2);
        n_sel += sel;
      }
      n_w = wave_sum_u64((uint64_t)n_sel);
      W1 = wave_sum_f64(S1);
      W2 = wave_sum_f64(S2);
    }
  }
  // ---- wave totals -> LDS, then thread 0 combines the waves in order
  const int wave = tid >> 6;
  DecWavePart& P = part[wave];
  uint64_t r;
  r = wave_sum_u64(n_rows_c); if (lane == 0) P.cnt[0] = r;
  r = wave_sum_u64(n_wnn); if (lane == 0) P.cnt[1] = r;
  if (lane == 0) P.cnt[2] = n_w;
  r = wave_sum_u64(s0); if (lane == 0) P.s[0] = r;
  r = wave_sum_u64(s1); if (lane == 0) P.s[1] = r;
  r = wave_sum_u64(s2); if (lane == 0) P.s[2] = r;
  r = wave_sum_u64(s3); if (lane == 0) P.s[3] = r;
  r = wave_sum_u64(a0); if (lane == 0) P.a[0] = r;
  r = wave_sum_u64(a1); if (lane == 0) P.a[1] = r;
  r = wave_sum_u64(a2); if (lane == 0) P.a[2] = r;
  r = wave_sum_u64(a3); if (lane == 0) P.a[3] = r;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t olo = (uint64_t)__shfl_down((unsigned long long)mn_lo, d, 64);
    const int64_t ohi = (int64_t)__shfl_down((long long)mn_hi, d, 64);
    if (less128(olo, ohi, mn_lo, mn_hi)) {
      mn_lo = olo;
      mn_hi = ohi;
    }
    const uint64_t xlo = (uint64_t)__shfl_down((unsigned long long)mx_lo, d, 64);
    const int64_t xhi = (int64_t)__shfl_down((long long)mx_hi, d, 64);
    if (less128(mx_lo, mx_hi, xlo, xhi)) {
      mx_lo = xlo;
      mx_hi = xhi;
    }
  }
  if (lane == 0) {
    P.min_lo = mn_lo;
    P.min_hi = mn_hi;
    P.max_lo = mx_lo;
    P.max_hi = mx_hi;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    if (stats_on && n_w > 0) {
      n = (double)n_w;
      mean = shift + W1 / n;
      m2 = W2 - W1 * W1 / n;
      m2 = (m2 < 0.0) ? 0.0 : m2;  // rounding
    }
    P.n = n;
    P.mean = mean;
    P.m2 = m2;
  }
  __syncthreads();
  if (tid == 0) {
    DecAcc out;
    dec_acc_init(out);
    double n = 0.0;
    uint64_t s[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int w = 0; w < kBlock / 64; ++w) {
      const DecWavePart& Q = part[w];
      out.n_rows += (int64_t)Q.cnt[0];
      out.n_wnn += (int64_t)Q.cnt[1];
      out.n_sel += (int64_t)Q.cnt[2];
      for (int j = 0; j < 4; ++j) {
        s[j] += Q.s[j];
        a[j] += Q.a[j];
      }
      if (less128(Q.min_lo, Q.min_hi, out.min_lo, out.min_hi)) {
        out.min_lo = Q.min_lo;
        out.min_hi = Q.min_hi;
      }
      if (less128(out.max_lo, out.max_hi, Q.max_lo, Q.max_hi)) {
        out.max_lo = Q.max_lo;
        out.max_hi = Q.max_hi;
      }
      moments_merge(n, out.mean, out.m2, Q.n, Q.mean, Q.m2);
    }
    // the limb sums of the block's rows (each below 2^63 in magnitude), recombined exactly
    for (int j = 0; j < 4; ++j) {
      add_limb192(out.sum, s[j], j == 3 && (int64_t)s[3] < 0, j);
      add_limb192(out.abs, a[j], false, j);
    }
    partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = out;
  }
}

// One block per task: the task's block partials merged in a fixed order, then folded into the
// running accumulator (batch order).
__global__ __launch_bounds__(kBlock) void dq_scan_dec_reduce_kernel(const DecAcc* __restrict__ partials,
                                                                    int blocks_per_task, DecAcc* acc) {
  const DecAcc* p = partials + (int64_t)blockIdx.x * blocks_per_task;
  __shared__ DecAcc slot[kBlock];
  const int k = (blocks_per_task + kBlock - 1) / kBlock;
  const int b0 = threadIdx.x * k;
  DecAcc a;
  dec_acc_init(a);
  for (int b = b0; b < b0 + k && b < blocks_per_task; ++b) dec_acc_merge(a, p[b]);
  slot[threadIdx.x] = a;
  __syncthreads();
  for (int s = 1; s < kBlock; s <<= 1) {
    if ((threadIdx.x % (2 * s)) == 0) dec_acc_merge(slot[threadIdx.x], slot[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    DecAcc run = acc[blockIdx.x];
    dec_acc_merge(run, slot[0]);
    acc[blockIdx.x] = run;
  }
}

__global__ void dq_init_dec_acc_kernel(DecAcc* acc, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    DecAcc a;
    dec_acc_init(a);
    acc[i] = a;
  }
}

// Cast(DecimalType(p, s) -> DoubleType) of a column: one row per lane; the validity bytes of a
// wave's 64 rows come from one ballot, written by its first eight lanes.
__global__ __launch_bounds__(kBlock) void dq_cast_decimal_kernel(DevColumn src, int scale, int64_t n_rows,
                                                                 double* __restrict__ out, uint8_t* __restrict__ out_valid) {
  const dq_v4u* __restrict__ values = static_cast<const dq_v4u*>(src.values);
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n_rows; base += (int64_t)gridDim.x * kBlock) {
    const int64_t r = base + threadIdx.x;
    const bool in = r < n_rows;
    const int64_t rc = in ? r : 0;
    const dq_v4u v = values[rc];
    bool valid = src.validity ? ((src.validity[rc >> 3] >> (rc & 7)) & 1u) != 0u : true;
    valid = valid && in;
    const uint64_t lo = (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    const int64_t hi = (int64_t)((uint64_t)v[2] | ((uint64_t)v[3] << 32));
    const double x = cast_row(lo, hi, scale, valid);
    if (in) out[r] = valid ? x : 0.0;
    const uint64_t bits = __ballot(valid);
    const int64_t r8 = (r - lane) + (int64_t)lane * 8;  // first row of this lane's validity byte
    if (lane < 8 && r8 < n_rows) out_valid[r8 >> 3] = (uint8_t)(bits >> (8 * lane));
  }
}

// ----------------------------------------------------------------------------- launchers
hipError_t launch_scan_dec(const DecTask* d_tasks, int n_tasks, const DevColumn* d_cols, const DevMask* d_masks,
                           int64_t n_rows, int blocks_per_task, DecAcc* d_partials, DecAcc* d_acc,
                           uint32_t* d_hll_regs, hipStream_t stream) {
  if (n_tasks <= 0 || n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_scan_dec_kernel, dim3(blocks_per_task, n_tasks), dim3(kBlock), 0, stream, d_tasks, d_cols,
                     d_masks, n_rows, d_partials, d_hll_regs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dq_scan_dec_reduce_kernel, dim3(n_tasks), dim3(kBlock), 0, stream, d_partials, blocks_per_task,
                     d_acc);
  return hipGetLastError();
}

hipError_t launch_init_dec_acc(DecAcc* d_acc, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_init_dec_acc_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_acc, n);
  return hipGetLastError();
}

int scan_dec_blocks_per_cu() {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(&dq_scan_dec_kernel), kBlock, 0) !=
          hipSuccess ||
      nb < 1)
    return 0;
  return nb;
}

hipError_t launch_cast_decimal(const DevColumn& src, int scale, int64_t n_rows, double* d_values, uint8_t* d_validity,
                               hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n_rows + kBlock - 1) / kBlock, 1 << 16);
  hipLaunchKernelGGL(dq_cast_decimal_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, scale, n_rows,
                     d_values, d_validity);
  return hipGetLastError();
}

}  // namespace dq
