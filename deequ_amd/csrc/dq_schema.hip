// dq_schema.hip -- RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala:183-281) on
// string-typed Arrow columns: one Kleene conjunction per row, then the rows that are TRUE
// (validRows, cast) and the rows that are FALSE (invalidRows, as they came) as new columns.
//
//   evaluate  blockIdx.y = definition, blockIdx.x = row range; a wave owns 64 consecutive rows and
//             writes the definition's FALSE bits and NULL bits of those rows as two 64-bit words
//             (__ballot).  No atomics anywhere: every word has one writer.  Int and decimal
//             definitions also write the parsed value of every row into a dense scratch column.
//   combine   folds the definitions' words into the `valid` and `invalid` bitmaps and their per-word
//             popcounts (scanned in place by the tree's own scan_exclusive_u32, dq_freq.hip).
//   select    source-row indices of the set bits, in row order: one lane per row.
//   gather    one lane per OUTPUT row reading sel[o]: fixed-width values, bit columns (bool values,
//             validity: a 64-bit word per 64 output rows by __ballot), utf8 lengths (scanned into
//             the new offsets) and bytes.  A NULL cell has length 0 and copies nothing.
//
// A utf8 row's bytes are only ever addressed inside [offsets[r], offsets[r + 1]): the evaluate
// kernel reads them through a buffer resource that spans exactly the batch's slice of the heap,
// with 16-byte loads while 16 bytes of the row remain, then 4, then 1 (as dq_regex_kernel does).
#include "dq_internal.h"
#include "dq_regex.h"
#include "dq_schema.h"

namespace dq {

using namespace schema;

namespace {

__device__ inline bool bit_at(const uint8_t* bm, int64_t row) { return (bm[row >> 3] >> (row & 7)) & 1u; }

__device__ inline uint32_t first_byte_step(uint32_t c) {  // UTF8String.numBytesForFirstByte (dq_pair.hip)
  return c < 0xC0u ? 1u : c < 0xE0u ? 2u : c < 0xF0u ? 3u : c < 0xF8u ? 4u : c < 0xFCu ? 5u : c < 0xFEu ? 6u : 1u;
}

__device__ __forceinline__ uint32_t step4(const uint8_t* cmap, const uint16_t* table, uint32_t s, uint32_t w) {
  const uint32_t c0 = cmap[w & 255u], c1 = cmap[(w >> 8) & 255u], c2 = cmap[(w >> 16) & 255u], c3 = cmap[w >> 24];
  s = table[s + c0];
  s = table[s + c1];
  s = table[s + c2];
  return table[s + c3];
}

// UTF8String.numChars as a byte stream: `skip` continuation bytes are passed over, the next byte
// is a first byte and counts (the walk i += numBytesForFirstByte(b[i]) of MinLength / MaxLength).
__device__ __forceinline__ void count1(uint32_t c, uint32_t& chars, uint32_t& skip) {
  if (skip) {
    --skip;
  } else {
    ++chars;
    skip = first_byte_step(c) - 1u;
  }
}
__device__ __forceinline__ void count4(uint32_t w, uint32_t& chars, uint32_t& skip) {
  count1(w & 255u, chars, skip);
  count1((w >> 8) & 255u, chars, skip);
  count1((w >> 16) & 255u, chars, skip);
  count1(w >> 24, chars, skip);
}

// Bytes of one row through the heap's buffer resource (index < row length: inside the row).
struct RowSrc {
  __amdgpu_buffer_rsrc_t rs;
  int32_t at;
  __device__ uint32_t operator[](int32_t i) const { return __builtin_amdgcn_raw_buffer_load_b8(rs, at + i, 0, 0); }
};

}  // namespace

__global__ __launch_bounds__(kBlock) void dq_schema_eval_kernel(const DevDef* __restrict__ defs,
                                                                const DevCol* __restrict__ cols,
                                                                const uint8_t* __restrict__ dfas, int64_t n_rows,
                                                                int64_t n_words, uint64_t* false_words,
                                                                uint64_t* null_words, uint8_t* scratch,
                                                                uint32_t* unsupported) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const DevDef def = defs[blockIdx.y];
  const bool walk = (def.flags & DF_MATCH) != 0;
  const bool count = (def.flags & (DF_MIN | DF_MAX)) != 0;
  uint32_t n_cols = 0, start_row = 0;
  if (walk) {  // (uniform over the workgroup)
    const uint32_t* img = reinterpret_cast<const uint32_t*>(dfas + def.dfa_off);
    n_cols = img[1];
    start_row = img[2];
    const uint32_t words = (256u + 2u * img[3] + 3u) >> 2;
    const uint32_t* src = img + regex::kRegexHeaderBytes / 4;
    uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
    for (uint32_t i = threadIdx.x; i < words; i += kBlock) dst[i] = src[i];
  }
  __syncthreads();
  const uint8_t* cmap = lds;
  const uint16_t* table = reinterpret_cast<const uint16_t*>(lds + 256);

  const DevCol col = cols[def.column];
  const int32_t heap_lo = col.offsets[0];
  const uint32_t heap_len = (uint32_t)(col.offsets[n_rows] - heap_lo);
  // the batch's slice of the heap as a bounds-checked buffer: a load outside it reads zeros
  const uint8_t* heap = static_cast<const uint8_t*>(col.values) + ((int64_t)heap_lo - col.heap_base);
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(heap), 0, (int)heap_len, 0x00020000);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t* fw_out = false_words + (int64_t)blockIdx.y * n_words;
  uint64_t* nw_out = null_words + (int64_t)blockIdx.y * n_words;
  int32_t* out32 = reinterpret_cast<int32_t*>(scratch + def.scratch_off);
  int64_t* out64 = reinterpret_cast<int64_t*>(scratch + def.scratch_off);

  for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + wave; w < n_words; w += (int64_t)gridDim.x * (kBlock / 64)) {
    const int64_t row = w * 64 + lane;
    bool f = false, u = false, unsup = false;
    if (row < n_rows) {
      const bool valid = !col.validity || bit_at(col.validity, col.bit_offset + row);
      int64_t parsed = 0;
      if (!valid) {
        f = (def.flags & DF_NOT_NULL) != 0;
        // line 246: colIsNull.isNull is FALSE, colAsInt >= minValue is NULL: the conjunct is NULL
        u = def.kind == DEF_INT && (def.flags & DF_MIN);
      } else {
        const int32_t b = col.offsets[row] - heap_lo, e = col.offsets[row + 1] - heap_lo;
        if (def.kind == DEF_INT) {
          int32_t v = 0;
          const bool ok = parse_int32(RowSrc{rs, b}, e - b, &v);
          f = !ok || ((def.flags & DF_MIN) && v < def.lo) || ((def.flags & DF_MAX) && v > def.hi);
          parsed = ok ? v : 0;
        } else if (def.kind == DEF_DECIMAL) {
          int64_t v = 0;
          const int32_t r = parse_decimal(RowSrc{rs, b}, e - b, def.precision, def.scale, &v);
          f = r == CELL_INVALID;
          unsup = r == CELL_UNSUPPORTED;
          parsed = r == CELL_VALID ? v : 0;
        } else {
          uint32_t s = start_row, chars = 0, skip = 0;
          int32_t p = b;
          while ((count || (walk && s != regex::kRegexAccept)) && e - p >= 16) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, p, 0, 0);
            if (walk) {  // (the accept state is absorbing: stepping on is harmless)
              s = step4(cmap, table, s, v[0]);
              s = step4(cmap, table, s, v[1]);
              s = step4(cmap, table, s, v[2]);
              s = step4(cmap, table, s, v[3]);
            }
            if (count) {
              count4(v[0], chars, skip);
              count4(v[1], chars, skip);
              count4(v[2], chars, skip);
              count4(v[3], chars, skip);
            }
            p += 16;
          }
          while ((count || (walk && s != regex::kRegexAccept)) && e - p >= 4) {
            const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(rs, p, 0, 0);
            if (walk) s = step4(cmap, table, s, v);
            if (count) count4(v, chars, skip);
            p += 4;
          }
          while ((count || (walk && s != regex::kRegexAccept)) && p < e) {
            const uint32_t c = __builtin_amdgcn_raw_buffer_load_b8(rs, p, 0, 0);
            if (walk) s = regex::regex_step(cmap, table, s, c);
            if (count) count1(c, chars, skip);
            ++p;
          }
          f = ((def.flags & DF_MIN) && (int64_t)chars < (int64_t)def.lo) ||
              ((def.flags & DF_MAX) && (int64_t)chars > (int64_t)def.hi) ||
              (walk && !regex::regex_finish(table, n_cols, s));
        }
      }
      if (def.kind == DEF_INT) out32[row] = (int32_t)parsed;
      else if (def.kind == DEF_DECIMAL) out64[row] = parsed;
    }
    const uint64_t fw = __ballot(f), nw = __ballot(u), uw = __ballot(unsup);
    if (lane == 0) {
      fw_out[w] = fw;
      nw_out[w] = nw;
      if (uw) unsupported[blockIdx.y] = 1u;  // (every writer stores the same value)
    }
  }
}

// valid = no conjunct FALSE and none NULL; invalid = some conjunct FALSE.  cnt_*[n_words] = 0, so
// that the exclusive scan leaves the totals there.
__global__ __launch_bounds__(kBlock) void dq_schema_combine_kernel(const uint64_t* __restrict__ false_words,
                                                                   const uint64_t* __restrict__ null_words, int n_defs,
                                                                   int64_t n_rows, int64_t n_words, uint64_t* valid_bm,
                                                                   uint64_t* invalid_bm, uint32_t* cnt_valid,
                                                                   uint32_t* cnt_invalid) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w > n_words) return;
  if (w == n_words) {
    cnt_valid[w] = 0;
    cnt_invalid[w] = 0;
    return;
  }
  uint64_t inv = 0, nul = 0;
  for (int d = 0; d < n_defs; ++d) {
    inv |= false_words[(int64_t)d * n_words + w];
    nul |= null_words[(int64_t)d * n_words + w];
  }
  const int64_t left = n_rows - w * 64;
  const uint64_t in_range = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
  inv &= in_range;
  const uint64_t val = ~(inv | nul) & in_range;
  valid_bm[w] = val;
  invalid_bm[w] = inv;
  cnt_valid[w] = (uint32_t)__popcll(val);
  cnt_invalid[w] = (uint32_t)__popcll(inv);
}

// sel[pre[w] + rank of the row among its word's set bits] = row, for both bitmaps.
__global__ __launch_bounds__(kBlock) void dq_schema_select_kernel(const uint64_t* __restrict__ valid_bm,
                                                                  const uint64_t* __restrict__ invalid_bm,
                                                                  const uint32_t* __restrict__ pre_valid,
                                                                  const uint32_t* __restrict__ pre_invalid,
                                                                  int64_t n_rows, int32_t* sel_valid,
                                                                  int32_t* sel_invalid) {
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t w = row >> 6;
  const uint32_t b = (uint32_t)(row & 63);
  const uint64_t below = (1ull << b) - 1ull;
  const uint64_t v = valid_bm[w], i = invalid_bm[w];
  if ((v >> b) & 1ull) sel_valid[pre_valid[w] + (uint32_t)__popcll(v & below)] = (int32_t)row;
  if ((i >> b) & 1ull) sel_invalid[pre_invalid[w] + (uint32_t)__popcll(i & below)] = (int32_t)row;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void dq_schema_gather_fixed_kernel(const T* __restrict__ src,
                                                                        const int32_t* __restrict__ sel, int64_t m,
                                                                        T* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o < m) dst[o] = src[sel[o]];
}

// Output bit o = source bit (bit_offset + sel[o]); a wave assembles the word of its 64 output rows.
// dst holds ceil(m / 64) words (bits past m are 0).
__global__ __launch_bounds__(kBlock) void dq_schema_gather_bits_kernel(const uint8_t* __restrict__ src,
                                                                       int64_t bit_offset,
                                                                       const int32_t* __restrict__ sel, int64_t m,
                                                                       uint64_t* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool bit = o < m && bit_at(src, bit_offset + sel[o]);
  const uint64_t word = __ballot(bit);
  if ((threadIdx.x & 63u) == 0 && o < m) dst[o >> 6] = word;
}

// len[o] = byte length of the selected cell, 0 for a NULL one; len[m] = 0 (the scan's total slot).
__global__ __launch_bounds__(kBlock) void dq_schema_gather_len_kernel(DevCol col, const int32_t* __restrict__ sel,
                                                                      int64_t m, uint32_t* __restrict__ len) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (o > m) return;
  uint32_t l = 0;
  if (o < m) {
    const int64_t r = sel[o];
    if (!col.validity || bit_at(col.validity, col.bit_offset + r)) l = (uint32_t)(col.offsets[r + 1] - col.offsets[r]);
  }
  len[o] = l;
}

// Bytes of the selected cells to their new places.  A lane copies its own row when that is short;
// rows of more than kLongRow bytes are copied by the whole wave, one after another.
constexpr int32_t kLongRow = 64;
__global__ __launch_bounds__(kBlock) void dq_schema_gather_bytes_kernel(DevCol col, const int32_t* __restrict__ sel,
                                                                        int64_t m, const int32_t* __restrict__ new_offs,
                                                                        uint8_t* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint8_t* heap = static_cast<const uint8_t*>(col.values);
  int64_t from = 0;
  int32_t to = 0, len = 0;
  if (o < m) {
    to = new_offs[o];
    len = new_offs[o + 1] - to;  // 0 for a NULL cell: its source offsets are not even read
    if (len > 0) from = (int64_t)col.offsets[sel[o]] - col.heap_base;
  }
  if (len <= kLongRow)
    for (int32_t i = 0; i < len; ++i) dst[to + i] = heap[from + i];
  uint64_t todo = __ballot(len > kLongRow);
  while (todo) {
    const int src_lane = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const int64_t f = __shfl((long long)from, src_lane, 64);
    const int32_t t = __shfl(to, src_lane, 64), l = __shfl(len, src_lane, 64);
    for (int32_t i = (int32_t)lane; i < l; i += 64) dst[t + i] = heap[f + i];
  }
}

// ---------------------------------------------------------------- launchers
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

hipError_t launch_schema_eval(const DevDef* d_defs, int n_defs, const DevCol* d_cols, const uint8_t* d_dfas,
                              uint32_t lds_bytes, int64_t n_rows, int blocks_per_def, uint64_t* d_false,
                              uint64_t* d_null, uint8_t* d_scratch, uint32_t* d_unsupported, hipStream_t stream) {
  if (n_defs <= 0 || n_rows <= 0) return hipSuccess;
  const int64_t n_words = (n_rows + 63) / 64;
  hipLaunchKernelGGL(dq_schema_eval_kernel, dim3(blocks_per_def, n_defs), dim3(kBlock), lds_bytes, stream, d_defs,
                     d_cols, d_dfas, n_rows, n_words, d_false, d_null, d_scratch, d_unsupported);
  return hipGetLastError();
}

hipError_t launch_schema_combine(const uint64_t* d_false, const uint64_t* d_null, int n_defs, int64_t n_rows,
                                 uint64_t* d_valid_bm, uint64_t* d_invalid_bm, uint32_t* d_cnt_valid,
                                 uint32_t* d_cnt_invalid, hipStream_t stream) {
  const int64_t n_words = (n_rows + 63) / 64;
  hipLaunchKernelGGL(dq_schema_combine_kernel, dim3(blocks_for(n_words + 1)), dim3(kBlock), 0, stream, d_false, d_null,
                     n_defs, n_rows, n_words, d_valid_bm, d_invalid_bm, d_cnt_valid, d_cnt_invalid);
  return hipGetLastError();
}

hipError_t launch_schema_select(const uint64_t* d_valid_bm, const uint64_t* d_invalid_bm, const uint32_t* d_pre_valid,
                                const uint32_t* d_pre_invalid, int64_t n_rows, int32_t* d_sel_valid,
                                int32_t* d_sel_invalid, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_schema_select_kernel, dim3(blocks_for(n_rows)), dim3(kBlock), 0, stream, d_valid_bm,
                     d_invalid_bm, d_pre_valid, d_pre_invalid, n_rows, d_sel_valid, d_sel_invalid);
  return hipGetLastError();
}

hipError_t launch_schema_gather_fixed(const void* d_src, int width, const int32_t* d_sel, int64_t m, void* d_dst,
                                      hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  const dim3 grid(blocks_for(m)), block(kBlock);
  switch (width) {
    case 1:
      hipLaunchKernelGGL(dq_schema_gather_fixed_kernel<uint8_t>, grid, block, 0, stream,
                         static_cast<const uint8_t*>(d_src), d_sel, m, static_cast<uint8_t*>(d_dst));
      break;
    case 2:
      hipLaunchKernelGGL(dq_schema_gather_fixed_kernel<uint16_t>, grid, block, 0, stream,
                         static_cast<const uint16_t*>(d_src), d_sel, m, static_cast<uint16_t*>(d_dst));
      break;
    case 4:
      hipLaunchKernelGGL(dq_schema_gather_fixed_kernel<uint32_t>, grid, block, 0, stream,
                         static_cast<const uint32_t*>(d_src), d_sel, m, static_cast<uint32_t*>(d_dst));
      break;
    case 8:
      hipLaunchKernelGGL(dq_schema_gather_fixed_kernel<uint64_t>, grid, block, 0, stream,
                         static_cast<const uint64_t*>(d_src), d_sel, m, static_cast<uint64_t*>(d_dst));
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_schema_gather_bits(const uint8_t* d_src, int64_t bit_offset, const int32_t* d_sel, int64_t m,
                                     uint64_t* d_dst, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_schema_gather_bits_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, stream, d_src, bit_offset,
                     d_sel, m, d_dst);
  return hipGetLastError();
}

hipError_t launch_schema_gather_len(const DevCol& col, const int32_t* d_sel, int64_t m, uint32_t* d_len,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(dq_schema_gather_len_kernel, dim3(blocks_for(m + 1)), dim3(kBlock), 0, stream, col, d_sel, m,
                     d_len);
  return hipGetLastError();
}

hipError_t launch_schema_gather_bytes(const DevCol& col, const int32_t* d_sel, int64_t m, const int32_t* d_new_offs,
                                      uint8_t* d_dst, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_schema_gather_bytes_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, stream, col, d_sel, m,
                     d_new_offs, d_dst);
  return hipGetLastError();
}

}  // namespace dq
