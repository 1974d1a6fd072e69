// dq_take.hip -- take: rows of chunked Arrow columns gathered by global row index (dq_take.h,
// dq_take_api.inc).  The map kernel validates the indices and turns each into (chunk, local row)
// once; every column's gather then reads that map, so no gather kernel sees an index that was not
// checked.  An output row whose index is -1 has chunk -1: zeros in the value buffers, 0 in the bit
// buffers, length 0 in a utf8 column.
//
//   map     one lane per output row; the chunks' row prefix (at most 4097 entries) staged in LDS and
//           searched by bisection; per workgroup at most one atomic (the smallest bad position, else
//           the count of -1 rows).
//   fixed   one lane per output row, one load and one store of the cell's width (1, 2, 4, 8, 16 B).
//   bits    bool values and every validity buffer: a wave ballots the 64 rows of one output word
//           and lane 0 stores it, so the bits past the last row are 0.
//   utf8    per-row lengths (0 for a NULL or -1 row, whose offsets and bytes are never read), an
//           exclusive 64-bit scan (scan_exclusive_u64) into the new offsets, then the byte copy: a
//           short cell by its lane, a longer one by its wave, and the cells of kSplitBytes or more
//           -- listed by the length pass -- in pieces by workgroups of their own.  All three copy
//           through take::copy_plan: 16-byte units where source and destination are congruent mod
//           16, 4-byte units where congruent mod 4, single bytes otherwise and at the ends; never a
//           byte outside the cell.
#include "dq_internal.h"
#include "dq_take.h"

namespace dq {

namespace {

using take::Chunk;
using take::kRowsPerBlock;

struct alignas(8) Cell16u {  // a 16-byte cell at an address that is only 8-byte aligned
  uint64_t lo, hi;
};

// copy_plan's access on the device: one load and one store of the width.
struct DevCopy {
  const uint8_t* s;
  uint8_t* d;
  __device__ void operator()(int64_t off, int width) const {
    if (width == 16) *reinterpret_cast<uint4*>(d + off) = *reinterpret_cast<const uint4*>(s + off);
    else if (width == 4) *reinterpret_cast<uint32_t*>(d + off) = *reinterpret_cast<const uint32_t*>(s + off);
    else d[off] = s[off];
  }
};

__device__ inline bool bit_at(const uint8_t* __restrict__ bits, int64_t b) { return (bits[b >> 3] >> (b & 7)) & 1u; }

}  // namespace

// status[0] += rows whose index is -1; status[1] = min(status[1], smallest output position whose
// index is outside [-1, total)) (the caller sets it to ~0).
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_map_kernel(const int64_t* __restrict__ rows, int64_t m,
                                                                    const int64_t* __restrict__ prefix, int n_chunks,
                                                                    int32_t* __restrict__ chunk,
                                                                    int64_t* __restrict__ local,
                                                                    unsigned long long* status) {
  extern __shared__ int64_t s_prefix[];  // n_chunks + 1
  __shared__ unsigned long long s_bad[kRowsPerBlock / 64];
  __shared__ uint32_t s_null[kRowsPerBlock / 64];
  for (int i = threadIdx.x; i <= n_chunks; i += kRowsPerBlock) s_prefix[i] = prefix[i];
  __syncthreads();
  const int64_t total = s_prefix[n_chunks];
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  bool is_null = false, bad = false;
  if (o < m) {
    const int64_t idx = rows[o];
    int32_t c = -1;
    int64_t l = 0;
    if (idx == -1) {
      is_null = true;
    } else if (idx < 0 || idx >= total) {
      bad = true;
    } else {
      c = take::find_chunk(static_cast<const int64_t*>(s_prefix), n_chunks, idx);
      l = idx - s_prefix[c];
    }
    chunk[o] = c;
    local[o] = l;
  }
  const uint64_t nm = __ballot(is_null), bm = __ballot(bad);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_null[wave] = (uint32_t)__popcll(nm);
    s_bad[wave] = bm ? (unsigned long long)(o + __builtin_ctzll(bm)) : ~0ull;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long first_bad = ~0ull;
    uint32_t nulls = 0;
    for (int w = 0; w < kRowsPerBlock / 64; ++w) {
      first_bad = s_bad[w] < first_bad ? s_bad[w] : first_bad;
      nulls += s_null[w];
    }
    if (first_bad != ~0ull) atomicMin(&status[1], first_bad);  // (the count is not read after a bad index)
    else if (nulls) atomicAdd(&status[0], (unsigned long long)nulls);
  }
}

template <typename T>
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_fixed_kernel(const Chunk* __restrict__ chunks,
                                                                      const int32_t* __restrict__ chunk,
                                                                      const int64_t* __restrict__ local, int64_t m,
                                                                      T* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  if (o >= m) return;
  const int32_t c = chunk[o];
  T v{};
  if (c >= 0) v = reinterpret_cast<const T*>(chunks[c].values)[local[o]];
  dst[o] = v;
}

template <bool kValidity>
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_bits_kernel(const Chunk* __restrict__ chunks,
                                                                     const int32_t* __restrict__ chunk,
                                                                     const int64_t* __restrict__ local, int64_t m,
                                                                     uint64_t* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  bool bit = false;
  if (o < m) {
    const int32_t c = chunk[o];
    if (c >= 0) {
      const uint8_t* p = kValidity ? chunks[c].validity : chunks[c].values;
      bit = (kValidity && p == nullptr) ? true : bit_at(p, chunks[c].bit_offset + local[o]);
    }
  }
  const uint64_t word = __ballot(bit);
  if ((threadIdx.x & 63u) == 0u && o < m) dst[o >> 6] = word;
}

// len[o] = the bytes of output row o (o < m), len[m] = 0; the rows of kSplitBytes or more are
// appended to `split` as {row, length} (at most kMaxSplitCells; *n_split counts them all).
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_len_kernel(const Chunk* __restrict__ chunks,
                                                                    const int32_t* __restrict__ chunk,
                                                                    const int64_t* __restrict__ local, int64_t m,
                                                                    unsigned long long* __restrict__ len,
                                                                    take::Piece* __restrict__ split,
                                                                    unsigned long long* n_split) {
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  if (o > m) return;
  int64_t n = 0;
  if (o < m) {
    const int32_t c = chunk[o];
    if (c >= 0) {
      const Chunk k = chunks[c];
      const int64_t l = local[o];
      if (k.validity == nullptr || bit_at(k.validity, k.bit_offset + l)) {
        n = (int64_t)k.offsets[l + 1] - (int64_t)k.offsets[l];
        if (n < 0) n = 0;
      }
    }
  }
  len[o] = (unsigned long long)n;
  if (n >= take::kSplitBytes) {
    const unsigned long long at = atomicAdd(n_split, 1ull);
    if (at < (unsigned long long)take::kMaxSplitCells) split[at] = take::Piece{o, n};
  }
}

__global__ __launch_bounds__(kRowsPerBlock) void dq_take_offsets_kernel(const unsigned long long* __restrict__ scan,
                                                                        int64_t m, int32_t* __restrict__ offsets) {
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  if (o <= m) offsets[o] = (int32_t)scan[o];
}

// The cells below kSplitBytes: scan[o] = output row o's first heap byte, scan[o + 1] - scan[o] its
// length (0 for a NULL or -1 row, whose chunk is then not read).
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_bytes_kernel(const Chunk* __restrict__ chunks,
                                                                      const int32_t* __restrict__ chunk,
                                                                      const int64_t* __restrict__ local, int64_t m,
                                                                      const unsigned long long* __restrict__ scan,
                                                                      uint8_t* __restrict__ dst) {
  const int64_t o = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63u);
  int64_t n = 0;
  unsigned long long s = 0, d = 0;
  if (o < m) {
    const unsigned long long at = scan[o];
    n = (int64_t)(scan[o + 1] - at);
    if (n > 0) {
      const Chunk k = chunks[chunk[o]];
      s = (unsigned long long)reinterpret_cast<uintptr_t>(k.values + k.offsets[local[o]]);
      d = (unsigned long long)reinterpret_cast<uintptr_t>(dst + at);
    }
  }
  if (n > 0 && n < take::kWaveBytes) {
    DevCopy op{reinterpret_cast<const uint8_t*>((uintptr_t)s), reinterpret_cast<uint8_t*>((uintptr_t)d)};
    take::copy_plan((uintptr_t)s, (uintptr_t)d, n, 0, 1, op);
  }
  uint64_t by_wave = __ballot(n >= take::kWaveBytes && n < take::kSplitBytes);
  while (by_wave) {
    const int j = __builtin_ctzll(by_wave);
    by_wave &= by_wave - 1;
    const unsigned long long sj = __shfl(s, j), dj = __shfl(d, j);
    const int64_t nj = (int64_t)__shfl((unsigned long long)n, j);
    DevCopy op{reinterpret_cast<const uint8_t*>((uintptr_t)sj), reinterpret_cast<uint8_t*>((uintptr_t)dj)};
    take::copy_plan((uintptr_t)sj, (uintptr_t)dj, nj, lane, 64, op);
  }
}

// One workgroup per piece of a cell of kSplitBytes or more.
__global__ __launch_bounds__(kRowsPerBlock) void dq_take_pieces_kernel(const Chunk* __restrict__ chunks,
                                                                       const int32_t* __restrict__ chunk,
                                                                       const int64_t* __restrict__ local,
                                                                       const take::Piece* __restrict__ pieces,
                                                                       const unsigned long long* __restrict__ scan,
                                                                       uint8_t* __restrict__ dst) {
  const take::Piece p = pieces[blockIdx.x];
  const unsigned long long at = scan[p.row];
  const int64_t rest = (int64_t)(scan[p.row + 1] - at) - p.start;
  if (rest <= 0) return;
  const Chunk k = chunks[chunk[p.row]];
  const uint8_t* s = k.values + k.offsets[local[p.row]] + p.start;
  uint8_t* d = dst + at + p.start;
  DevCopy op{s, d};
  take::copy_plan(reinterpret_cast<uintptr_t>(s), reinterpret_cast<uintptr_t>(d),
                  rest < take::kSplitBytes ? rest : take::kSplitBytes, (int)threadIdx.x, kRowsPerBlock, op);
}

// ---------------------------------------------------------------- launchers
static unsigned row_blocks(int64_t rows) { return (unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock); }

hipError_t launch_take_map(const int64_t* d_rows, int64_t m, const int64_t* d_prefix, int n_chunks, int32_t* d_chunk,
                           int64_t* d_local, unsigned long long* d_status, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  if (n_chunks < 1 || n_chunks > take::kMaxChunks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dq_take_map_kernel, dim3(row_blocks(m)), dim3(kRowsPerBlock), (size_t)(n_chunks + 1) * sizeof(int64_t),
                     stream, d_rows, m, d_prefix, n_chunks, d_chunk, d_local, d_status);
  return hipGetLastError();
}

hipError_t launch_take_fixed(const take::Chunk* d_chunks, int width, bool aligned16, const int32_t* d_chunk,
                             const int64_t* d_local, int64_t m, void* d_dst, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  const dim3 grid(row_blocks(m)), block(kRowsPerBlock);
#define DQ_TAKE_FIXED(T)                                                                                          \
  hipLaunchKernelGGL(dq_take_fixed_kernel<T>, grid, block, 0, stream, d_chunks, d_chunk, d_local, m, static_cast<T*>(d_dst))
  switch (width) {
    case 1: DQ_TAKE_FIXED(uint8_t); break;
    case 2: DQ_TAKE_FIXED(uint16_t); break;
    case 4: DQ_TAKE_FIXED(uint32_t); break;
    case 8: DQ_TAKE_FIXED(uint64_t); break;
    case 16:
      if (aligned16) DQ_TAKE_FIXED(uint4);
      else DQ_TAKE_FIXED(Cell16u);
      break;
    default: return hipErrorInvalidValue;
  }
#undef DQ_TAKE_FIXED
  return hipGetLastError();
}

hipError_t launch_take_bits(const take::Chunk* d_chunks, bool validity, const int32_t* d_chunk, const int64_t* d_local,
                            int64_t m, uint64_t* d_dst, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  if (validity)
    hipLaunchKernelGGL(dq_take_bits_kernel<true>, dim3(row_blocks(m)), dim3(kRowsPerBlock), 0, stream, d_chunks, d_chunk,
                       d_local, m, d_dst);
  else
    hipLaunchKernelGGL(dq_take_bits_kernel<false>, dim3(row_blocks(m)), dim3(kRowsPerBlock), 0, stream, d_chunks, d_chunk,
                       d_local, m, d_dst);
  return hipGetLastError();
}

hipError_t launch_take_len(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local, int64_t m,
                           unsigned long long* d_len, take::Piece* d_split, unsigned long long* d_n_split,
                           hipStream_t stream) {
  if (m < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dq_take_len_kernel, dim3(row_blocks(m + 1)), dim3(kRowsPerBlock), 0, stream, d_chunks, d_chunk,
                     d_local, m, d_len, d_split, d_n_split);
  return hipGetLastError();
}

hipError_t launch_take_offsets(const unsigned long long* d_scan, int64_t m, int32_t* d_offsets, hipStream_t stream) {
  if (m < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dq_take_offsets_kernel, dim3(row_blocks(m + 1)), dim3(kRowsPerBlock), 0, stream, d_scan, m,
                     d_offsets);
  return hipGetLastError();
}

hipError_t launch_take_bytes(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local, int64_t m,
                             const unsigned long long* d_scan, uint8_t* d_dst, hipStream_t stream) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_take_bytes_kernel, dim3(row_blocks(m)), dim3(kRowsPerBlock), 0, stream, d_chunks, d_chunk,
                     d_local, m, d_scan, d_dst);
  return hipGetLastError();
}

hipError_t launch_take_pieces(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local,
                              const take::Piece* d_pieces, int64_t n_pieces, const unsigned long long* d_scan,
                              uint8_t* d_dst, hipStream_t stream) {
  if (n_pieces <= 0) return hipSuccess;
  hipLaunchKernelGGL(dq_take_pieces_kernel, dim3((unsigned)n_pieces), dim3(kRowsPerBlock), 0, stream, d_chunks, d_chunk,
                     d_local, d_pieces, d_scan, d_dst);
  return hipGetLastError();
}

}  // namespace dq
