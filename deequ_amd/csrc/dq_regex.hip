// dq_regex.hip -- PatternMatch (PatternMatch.scala:37-55) on a utf8 column:
//   matches = sum(conditionalSelection(when(regexp_extract(col, pattern, 0) != "", 1).otherwise(0), where))
//   count   = conditionalCount(where)
// The pattern is a search DFA compiled on the host (dq_regex.h / dq_regex.cpp).  blockIdx.y is a
// task {column, where mask, DFA}, blockIdx.x a contiguous row range.  A workgroup stages its task's
// byte -> column map (256 B) and transition table (at most regex::kMaxTableBytes) into LDS once;
// then one lane walks one row: 16 bytes per buffer load (4, then 1 for the tail -- never a byte
// outside the row), two LDS reads per byte, and it stops loading once it is in the accept state
// (checked per load, the state being absorbing).  Two integers per task -- rows in scope, rows that
// match -- folded by wave reductions and one atomic pair per wave: order independent, bit-exact.
#include "dq_internal.h"
#include "dq_regex.h"

namespace dq {

namespace {

__device__ inline bool bit_at(const uint8_t* bm, int64_t row) { return (bm[row >> 3] >> (row & 7)) & 1u; }
__device__ inline bool word_bit(const uint64_t* w, int64_t row) { return (w[row >> 6] >> (row & 63)) & 1ull; }

__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
  return v;
}

__device__ __forceinline__ uint32_t step4(const uint8_t* cmap, const uint16_t* table, uint32_t s, uint32_t w) {
  // the four column lookups do not depend on the state: issued together, ahead of the chain
  const uint32_t c0 = cmap[w & 255u], c1 = cmap[(w >> 8) & 255u], c2 = cmap[(w >> 16) & 255u], c3 = cmap[w >> 24];
  s = table[s + c0];
  s = table[s + c1];
  s = table[s + c2];
  return table[s + c3];
}

// The workgroup's copy of an image's byte map and table (the image is padded to 16 bytes, so whole
// words cover it); the caller synchronises.
__device__ inline void stage_image(const uint32_t* img, uint32_t n_entries, uint8_t* lds) {
  const uint32_t words = (256u + 2u * n_entries + 3u) >> 2;
  const uint32_t* src = img + regex::kRegexHeaderBytes / 4;
  uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
  for (uint32_t i = threadIdx.x; i < words; i += kBlock) dst[i] = src[i];
}

// One row's bytes [b, e) of the heap behind `rs`, from the start row: 16 bytes per load, then 4,
// then 1 -- never a byte outside the row -- and no further load once the state is the accept row.
__device__ __forceinline__ bool walk_row(const __amdgpu_buffer_rsrc_t rs, const uint8_t* cmap, const uint16_t* table,
                                         uint32_t n_cols, uint32_t start_row, int32_t b, int32_t e) {
  uint32_t s = start_row;
  int32_t p = b;
  while (s != regex::kRegexAccept && e - p >= 16) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, p, 0, 0);
    s = step4(cmap, table, s, v[0]);
    s = step4(cmap, table, s, v[1]);
    s = step4(cmap, table, s, v[2]);
    s = step4(cmap, table, s, v[3]);
    p += 16;
  }
  while (s != regex::kRegexAccept && e - p >= 4) {
    s = step4(cmap, table, s, __builtin_amdgcn_raw_buffer_load_b32(rs, p, 0, 0));
    p += 4;
  }
  while (s != regex::kRegexAccept && p < e) {
    s = regex::regex_step(cmap, table, s, __builtin_amdgcn_raw_buffer_load_b8(rs, p, 0, 0));
    ++p;
  }
  return regex::regex_finish(table, n_cols, s);
}

}  // namespace

// LIKE / RLIKE of a predicate: blockIdx.y is a match task {column, DFA}; the workgroup stages the
// image as dq_regex_kernel does, then each wave takes 64 consecutive rows (word w of the mask), one
// lane walks one row, and lane 0 stores the wave's ballot: bit r = row r matched; a NULL row and a
// lane past n_rows give 0.  No atomics: every word is written once, by one wave.
__global__ __launch_bounds__(kBlock) void dq_match_mask_kernel(const MatchTask* __restrict__ tasks,
                                                               const DevColumn* __restrict__ cols,
                                                               const uint8_t* __restrict__ dfas, int64_t n_rows,
                                                               uint64_t* __restrict__ out, int64_t words_per_mask) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const MatchTask task = tasks[blockIdx.y];
  const uint32_t* img = reinterpret_cast<const uint32_t*>(dfas + task.dfa_off);
  const uint32_t n_cols = img[1], start_row = img[2], n_entries = img[3];
  stage_image(img, n_entries, lds);
  __syncthreads();
  const uint8_t* cmap = lds;
  const uint16_t* table = reinterpret_cast<const uint16_t*>(lds + 256);

  const DevColumn& col = cols[task.column];
  const uint32_t heap_end = (uint32_t)col.offsets[n_rows];
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(static_cast<const uint8_t*>(col.values)), 0, (int)heap_end, 0x00020000);
  const int lane = threadIdx.x & 63;
  const int64_t n_words = (n_rows + 63) >> 6;
  uint64_t* out_m = out + (int64_t)blockIdx.y * words_per_mask;
  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w < n_words;
       w += (int64_t)gridDim.x * (kBlock / 64)) {
    const int64_t row = (w << 6) + lane;
    bool hit = false;
    if (row < n_rows && (!col.validity || bit_at(col.validity, row)))
      hit = walk_row(rs, cmap, table, n_cols, start_row, col.offsets[row], col.offsets[row + 1]);
    const uint64_t word = __ballot(hit);
    if (lane == 0) out_m[w] = word;
  }
}

hipError_t launch_match_mask(const MatchTask* d_tasks, int n_tasks, const DevColumn* d_cols, const uint8_t* d_dfas,
                             uint32_t lds_bytes, int64_t n_rows, uint64_t* d_out, int64_t words_per_mask,
                             hipStream_t stream) {
  if (n_tasks <= 0 || n_rows <= 0) return hipSuccess;
  const int64_t n_words = (n_rows + 63) >> 6;
  int64_t blocks = (n_words + 3) / 4;
  const int64_t cap = std::max<int64_t>(1, 4096 / n_tasks);
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(dq_match_mask_kernel, dim3((unsigned)blocks, n_tasks), dim3(kBlock), lds_bytes, stream, d_tasks,
                     d_cols, d_dfas, n_rows, d_out, words_per_mask);
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void dq_regex_kernel(const RegexTask* __restrict__ tasks,
                                                          const DevColumn* __restrict__ cols,
                                                          const DevMask* __restrict__ masks,
                                                          const uint8_t* __restrict__ dfas, int64_t n_rows,
                                                          unsigned long long* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const RegexTask task = tasks[blockIdx.y];
  const uint32_t* img = reinterpret_cast<const uint32_t*>(dfas + task.dfa_off);
  const uint32_t n_cols = img[1], start_row = img[2], n_entries = img[3];
  {  // (the image is padded to 16 bytes, so whole words cover it)
    const uint32_t words = (256u + 2u * n_entries + 3u) >> 2;
    const uint32_t* src = img + regex::kRegexHeaderBytes / 4;
    uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
    for (uint32_t i = threadIdx.x; i < words; i += kBlock) dst[i] = src[i];
  }
  __syncthreads();
  const uint8_t* cmap = lds;
  const uint16_t* table = reinterpret_cast<const uint16_t*>(lds + 256);

  const DevColumn& col = cols[task.column];
  const uint64_t* wt = task.where_mask >= 0 ? masks[task.where_mask].t : nullptr;
  const uint8_t* vals = static_cast<const uint8_t*>(col.values);
  const int64_t per_block = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per_block;
  const int64_t r1 = min(r0 + per_block, n_rows);
  // the string heap as a bounds-checked buffer: a load past its end reads zeros, never memory
  const uint32_t heap_end = (uint32_t)col.offsets[n_rows];
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(vals), 0, (int)heap_end, 0x00020000);
  uint64_t cnt = 0, hits = 0;
  for (int64_t row = r0 + threadIdx.x; row < r1; row += kBlock) {
    // conditionalCount: rows whose filter is TRUE; a NULL string is in scope and matches nothing
    if (wt && !word_bit(wt, row)) continue;
    ++cnt;
    if (col.validity && !bit_at(col.validity, row)) continue;
    const int32_t b = col.offsets[row], e = col.offsets[row + 1];
    uint32_t s = start_row;
    int32_t p = b;
    while (s != regex::kRegexAccept && e - p >= 16) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, p, 0, 0);
      s = step4(cmap, table, s, v[0]);
      s = step4(cmap, table, s, v[1]);
      s = step4(cmap, table, s, v[2]);
      s = step4(cmap, table, s, v[3]);
      p += 16;
    }
    while (s != regex::kRegexAccept && e - p >= 4) {
      s = step4(cmap, table, s, __builtin_amdgcn_raw_buffer_load_b32(rs, p, 0, 0));
      p += 4;
    }
    while (s != regex::kRegexAccept && p < e) {
      s = regex::regex_step(cmap, table, s, __builtin_amdgcn_raw_buffer_load_b8(rs, p, 0, 0));
      ++p;
    }
    hits += regex::regex_finish(table, n_cols, s) ? 1u : 0u;
  }
  cnt = wave_sum(cnt);
  hits = wave_sum(hits);
  if ((threadIdx.x & 63) == 0 && cnt) {
    unsigned long long* o = out + (int64_t)blockIdx.y * 2;
    atomicAdd(&o[0], (unsigned long long)cnt);
    if (hits) atomicAdd(&o[1], (unsigned long long)hits);
  }
}

hipError_t launch_regex(const RegexTask* d_tasks, int n_tasks, const DevColumn* d_cols, const DevMask* d_masks,
                        const uint8_t* d_dfas, uint32_t lds_bytes, int64_t n_rows, int blocks_per_task,
                        unsigned long long* d_out, hipStream_t stream) {
  if (n_tasks <= 0 || n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_regex_kernel, dim3(blocks_per_task, n_tasks), dim3(kBlock), lds_bytes, stream, d_tasks, d_cols,
                     d_masks, d_dfas, n_rows, d_out);
  return hipGetLastError();
}

}  // namespace dq
