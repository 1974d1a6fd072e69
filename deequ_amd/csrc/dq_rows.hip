// dq_rows.hip -- row-level outcomes: one nullable boolean per row and analyzer, as two bitmaps in
// the Arrow boolean layout (LSB first, 64-bit words): `value` (TRUE) and `valid` (not NULL).
//
//   combine  value = condition & selected, valid = selected.  The condition is what the analyzer
//            counts (a column's validity, a predicate's TRUE plane, a match mask, the frequency
//            probe's "count == 1" bits), selected the TRUE plane of its `where` (or every row).
//            A batch lands at its row offset in a bitmap pair that spans the whole table, so the
//            source words are shifted into place: one thread per destination word, which reads at
//            most two source words of each plane.  Only the first and the last destination word
//            can hold bits of other batches; those two are read, merged and written back, and the
//            batches of one bitmap run one after the other on the stream.
//   select   the ascending row indices of the rows whose outcome is FALSE / TRUE / NULL: the picked
//            bits of every word are counted, the counts scanned (scan_exclusive_u64), and one wave
//            per word scatters its rows -- lane r writes row 64 w + r at the word's base plus the
//            picked bits below r.  No atomics: every index has one place, whatever the schedule.
#include "dq_internal.h"

namespace dq {

namespace {

// Word j (rows [64 j, 64 j + 64)) of a source plane over n_rows rows: bits at and past n_rows are
// 0, as is every word outside the plane.  bytes: a bitmap at any byte address, (n_rows + 7) / 8
// bytes long; words: 64-bit words; neither: all ones.
__device__ inline uint64_t plane_word(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ words, int64_t j,
                                      int64_t n_rows) {
  if (j < 0 || (j << 6) >= n_rows) return 0ull;
  uint64_t v = ~0ull;
  if (words != nullptr) {
    v = words[j];
  } else if (bytes != nullptr) {
    const int64_t n_bytes = (n_rows + 7) >> 3;
    v = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t b = (j << 3) + k;
      if (b < n_bytes) v |= (uint64_t)bytes[b] << (8 * k);
    }
  }
  const int64_t rest = n_rows - (j << 6);
  return rest < 64 ? v & ((1ull << rest) - 1ull) : v;
}

// The 64 source bits that land in destination word `first + j`, the plane being shifted up by sh.
__device__ inline uint64_t shifted_word(const uint8_t* bytes, const uint64_t* words, int64_t j, uint32_t sh,
                                        int64_t n_rows) {
  const uint64_t hi = plane_word(bytes, words, j, n_rows);
  if (sh == 0u) return hi;
  return (hi << sh) | (plane_word(bytes, words, j - 1, n_rows) >> (64u - sh));
}

__device__ inline uint64_t picked_word(const uint64_t* __restrict__ value, const uint64_t* __restrict__ valid,
                                       int64_t w, int64_t n_rows, int which) {
  const uint64_t t = value[w], v = valid[w];
  uint64_t p = 0ull;
  if (which & DQ_ROWS_FALSE) p |= ~t & v;
  if (which & DQ_ROWS_TRUE) p |= t & v;
  if (which & DQ_ROWS_NULL) p |= ~v;
  const int64_t rest = n_rows - (w << 6);
  return rest < 64 ? p & ((1ull << rest) - 1ull) : p;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void dq_rows_combine_kernel(const uint8_t* __restrict__ cond_bytes,
                                                                 const uint64_t* __restrict__ cond_words,
                                                                 const uint64_t* __restrict__ sel_words, int64_t n_rows,
                                                                 int64_t out_off, uint64_t* value, uint64_t* valid) {
  const int64_t first = out_off >> 6, last = (out_off + n_rows - 1) >> 6;
  const uint32_t sh = (uint32_t)(out_off & 63);
  for (int64_t d = first + (int64_t)blockIdx.x * kBlock + threadIdx.x; d <= last; d += (int64_t)gridDim.x * kBlock) {
    const int64_t j = d - first;
    const uint64_t s = shifted_word(nullptr, sel_words, j, sh, n_rows);
    const uint64_t c = shifted_word(cond_bytes, cond_words, j, sh, n_rows) & s;
    // the destination bits this batch owns: [out_off, out_off + n_rows) within word d
    uint64_t mine = ~0ull;
    if (d == first) mine &= ~0ull << sh;
    const int64_t end = out_off + n_rows - (d << 6);
    if (end < 64) mine &= (1ull << end) - 1ull;
    if (mine == ~0ull) {
      value[d] = c;
      valid[d] = s;
    } else {  // (c and s are 0 outside `mine`: the planes end at n_rows and the shift brings in zeros)
      value[d] = (value[d] & ~mine) | c;
      valid[d] = (valid[d] & ~mine) | s;
    }
  }
}

hipError_t launch_rows_combine(const uint8_t* cond_bytes, const uint64_t* cond_words, const uint64_t* sel_words,
                               int64_t n_rows, int64_t out_off, uint64_t* d_value, uint64_t* d_valid,
                               hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const int64_t n_dst = ((out_off + n_rows - 1) >> 6) - (out_off >> 6) + 1;
  const int64_t blocks = std::min<int64_t>((n_dst + kBlock - 1) / kBlock, 2048);
  hipLaunchKernelGGL(dq_rows_combine_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, cond_bytes, cond_words,
                     sel_words, n_rows, out_off, d_value, d_valid);
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void dq_rows_select_count_kernel(const uint64_t* __restrict__ value,
                                                                      const uint64_t* __restrict__ valid,
                                                                      int64_t n_rows, int which,
                                                                      unsigned long long* __restrict__ counts) {
  const int64_t n_words = (n_rows + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w <= n_words; w += (int64_t)gridDim.x * kBlock)
    counts[w] = w < n_words ? (unsigned long long)__popcll(picked_word(value, valid, w, n_rows, which)) : 0ull;
}

__global__ __launch_bounds__(kBlock) void dq_rows_select_scatter_kernel(const uint64_t* __restrict__ value,
                                                                        const uint64_t* __restrict__ valid,
                                                                        int64_t n_rows, int which,
                                                                        const unsigned long long* __restrict__ base,
                                                                        int64_t* __restrict__ out, int64_t capacity) {
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t n_words = (n_rows + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_words;
       w += (int64_t)gridDim.x * (kBlock / 64)) {
    const uint64_t p = picked_word(value, valid, w, n_rows, which);
    if (!((p >> lane) & 1ull)) continue;
    const int64_t at = (int64_t)base[w] + __popcll(p & ((1ull << lane) - 1ull));
    if (at < capacity) out[at] = (w << 6) + lane;
  }
}

hipError_t launch_rows_select_count(const uint64_t* d_value, const uint64_t* d_valid, int64_t n_rows, int which,
                                    unsigned long long* d_counts, hipStream_t stream) {
  const int64_t n = ((n_rows + 63) >> 6) + 1;
  const int64_t blocks = std::min<int64_t>((n + kBlock - 1) / kBlock, kRowsSelectMaxBlocks);
  hipLaunchKernelGGL(dq_rows_select_count_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d_value, d_valid,
                     n_rows, which, d_counts);
  return hipGetLastError();
}

hipError_t launch_rows_select_scatter(const uint64_t* d_value, const uint64_t* d_valid, int64_t n_rows, int which,
                                      const unsigned long long* d_base, int64_t* d_out, int64_t capacity,
                                      hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const int64_t n_words = (n_rows + 63) >> 6;
  const int64_t blocks = std::min<int64_t>((n_words + 3) / 4, kRowsSelectMaxBlocks);
  hipLaunchKernelGGL(dq_rows_select_scatter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d_value, d_valid,
                     n_rows, which, d_base, d_out, capacity);
  return hipGetLastError();
}

}  // namespace dq
