// dq_pred.hip -- generic predicate evaluation into row masks.
//
// Spark parses every Compliance predicate and `where` filter with `expr(String)`
// (Compliance.scala:49, Analyzer.scala:413-432) and evaluates it per row with SQL
// three-valued logic.  The fused scan kernel evaluates the common single-comparison forms
// inline; every other predicate of a plan is run here first, once per batch, by a small
// postfix interpreter (the plan's validated dq_pred_insn program).  Each wave evaluates 64
// consecutive rows and writes two 64-bit ballot words: TRUE bits and NOT-NULL bits.  The scan
// kernel then reads those masks (2 bits per row instead of the referenced columns' bytes).
// A LIKE / RLIKE of a program is not walked here: dq_match_mask_kernel (dq_regex.hip) has written
// one bit per row before this kernel starts, and the interpreter reads it (kPredMatch).
// The interpreter itself (types, three-valued logic, Spark 2.2's casts) is dq_predeval.h, shared
// with the host build the CPU tests check against the oracle.
#include "dq_predeval.h"

namespace dq {

template <bool CAST>
__global__ __launch_bounds__(kBlock) void dq_pred_kernel(const PredProgram* __restrict__ progs,
                                                         const PredInsn* __restrict__ insns,
                                                         const uint8_t* __restrict__ pool,
                                                         const DevColumn* __restrict__ cols,
                                                         int64_t n_rows, uint64_t* out,
                                                         int64_t words_per_mask,
                                                         const uint64_t* __restrict__ match_words) {
  const PredProgram prog = progs[blockIdx.y];
  const PredInsn* code = insns + prog.first;
  const int lane = threadIdx.x & 63;
  const int64_t n_words = (n_rows + 63) >> 6;
  uint64_t* out_t = out + (int64_t)(2 * blockIdx.y) * words_per_mask;
  uint64_t* out_n = out_t + words_per_mask;
  const MatchSource ms{match_words, words_per_mask, nullptr, nullptr};
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_words;
       w += (int64_t)gridDim.x * (kBlock / 64)) {
    const int64_t row = (w << 6) + lane;
    bool t = false, nn = false;
    if (row < n_rows) pred::eval_program<CAST>(code, prog.n, pool, cols, row, t, nn, ms);
    const uint64_t bt = __ballot(t);
    const uint64_t bn = __ballot(nn);
    if (lane == 0) {
      out_t[w] = bt;
      out_n[w] = bn;
    }
  }
}

// dst bit i = src bit (bit_offset + i): realigns a sliced Arrow bitmap so that bit 0 of
// byte 0 is row 0 of the batch.
__global__ void dq_realign_kernel(const uint8_t* __restrict__ src, int64_t bit_offset,
                                  int64_t n_bits, uint8_t* __restrict__ dst) {
  const int64_t n_bytes = (n_bits + 7) >> 3;
  const int64_t src_bytes = (bit_offset + n_bits + 7) >> 3;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bytes;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bit = bit_offset + (i << 3);
    const int64_t b = bit >> 3;
    const uint32_t sh = (uint32_t)(bit & 7);
    uint32_t v = src[b] >> sh;
    if (sh && b + 1 < src_bytes) v |= (uint32_t)src[b + 1] << (8 - sh);
    dst[i] = (uint8_t)v;
  }
}

hipError_t launch_predicates(const PredProgram* d_progs, int n_progs, const PredInsn* d_insns,
                             const uint8_t* d_pool, const DevColumn* d_cols, int64_t n_rows,
                             uint64_t* d_mask_words, int64_t words_per_mask, bool with_cast, hipStream_t stream,
                             const uint64_t* d_match_words) {
  if (n_progs <= 0 || n_rows <= 0) return hipSuccess;
  const int64_t n_words = (n_rows + 63) >> 6;
  int64_t blocks = (n_words + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  if (with_cast)
    hipLaunchKernelGGL(dq_pred_kernel<true>, dim3((unsigned)blocks, n_progs), dim3(kBlock), 0, stream,
                       d_progs, d_insns, d_pool, d_cols, n_rows, d_mask_words, words_per_mask, d_match_words);
  else
    hipLaunchKernelGGL(dq_pred_kernel<false>, dim3((unsigned)blocks, n_progs), dim3(kBlock), 0, stream,
                       d_progs, d_insns, d_pool, d_cols, n_rows, d_mask_words, words_per_mask, d_match_words);
  return hipGetLastError();
}

// The `where` of a frequency table (dq_freq_set_filter): a row takes part only where the filter is
// TRUE, and every frequency stage drops a row by the key columns' validity alone, so the filter's
// TRUE word is folded into the first key column's validity: out word w = TRUE word w & validity
// bits [64 w, 64 w + 64).  One wave per word, as dq_pred_kernel: lanes 0..7 load the word's
// validity bytes (the bitmap may start at any byte and end with the batch's last byte), lane 0
// stores the word.  The TRUE words are 0 at and past n_rows, so the bitmap is too; the word after
// the last is zeroed for readers of whole dwords.  *selected += the TRUE bits (numRows of the
// filtered data): one atomic per workgroup, an integer sum in any order.
__global__ __launch_bounds__(kBlock) void dq_freq_filter_kernel(const uint64_t* __restrict__ true_words,
                                                                const uint8_t* __restrict__ validity, int64_t n_rows,
                                                                uint64_t* __restrict__ out,
                                                                unsigned long long* selected) {
  __shared__ unsigned long long s_sel[kBlock / 64];
  const uint32_t lane = threadIdx.x & 63u;
  const int64_t n_words = (n_rows + 63) >> 6;
  const int64_t n_bytes = (n_rows + 7) >> 3;
  unsigned long long sel = 0;
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_words;
       w += (int64_t)gridDim.x * (kBlock / 64)) {
    const uint64_t t = true_words[w];
    uint64_t v = ~0ull;
    if (validity != nullptr) {
      const int64_t b = (w << 3) + lane;
      const uint32_t byte = (lane < 8u && b < n_bytes) ? validity[b] : 0u;
      uint32_t lo = 0u, hi = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)__builtin_amdgcn_readlane((int)byte, k) << (8 * k);
        hi |= (uint32_t)__builtin_amdgcn_readlane((int)byte, 4 + k) << (8 * k);
      }
      v = ((uint64_t)hi << 32) | lo;
    }
    if (lane == 0u) {
      out[w] = t & v;
      if (w == n_words - 1) out[n_words] = 0ull;
    }
    sel += (unsigned long long)__popcll(t);
  }
  if (lane == 0u) s_sel[threadIdx.x >> 6] = sel;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
    for (int k = 0; k < kBlock / 64; ++k) sum += s_sel[k];
    if (sum) atomicAdd(selected, sum);
  }
}

hipError_t launch_freq_filter(const uint64_t* d_true_words, const uint8_t* validity, int64_t n_rows, uint64_t* d_out,
                              unsigned long long* d_selected, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  const int64_t n_words = (n_rows + 63) >> 6;
  const int64_t blocks = std::min<int64_t>((n_words + 3) / 4, kFreqFilterMaxBlocks);
  hipLaunchKernelGGL(dq_freq_filter_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d_true_words, validity,
                     n_rows, d_out, d_selected);
  return hipGetLastError();
}

// offs[i] -= first: utf8 offsets of a host batch copied verbatim, rebased to its first byte
__global__ void dq_rebase_offsets_kernel(int32_t* __restrict__ offs, int64_t n, int32_t first) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    offs[i] -= first;
}

hipError_t launch_rebase_offsets(int32_t* d_offs, int64_t n, int32_t first, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dq_rebase_offsets_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_offs, n, first);
  return hipGetLastError();
}

hipError_t launch_realign_bitmap(const uint8_t* src, int64_t bit_offset, int64_t n_bits,
                                 uint8_t* dst, hipStream_t stream) {
  const int64_t n_bytes = (n_bits + 7) >> 3;
  if (n_bytes <= 0) return hipSuccess;
  int64_t blocks = (n_bytes + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(dq_realign_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src,
                     bit_offset, n_bits, dst);
  return hipGetLastError();
}

}  // namespace dq
