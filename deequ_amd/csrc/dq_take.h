// dq_take.h -- take: rows of chunked Arrow columns gathered by global row index (dq_take_*,
// include/deequ_amd.h "take").  Shared by the host runner (dq_take_api.inc), the gfx950 kernels
// (dq_take.hip) and the stand-alone host check (tools/take_check.cpp): the tiling constants, the
// structures the kernels address a column by, and the byte-copy addressing -- which bytes of a cell
// a lane touches and at which width -- as host/device functions, so that the kernels and the host
// check run one source.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef DQ_HD
#define DQ_HD __host__ __device__
#endif
#else
#ifndef DQ_HD
#define DQ_HD
#endif
#endif

namespace dq {
namespace take {

// ---------------------------------------------------------------- tiling
constexpr int kRowsPerBlock = 256;  // output rows of one workgroup (one lane each; 4 output words)
constexpr int kScanTile = 4096;     // entries of one tile of scan_exclusive_u64 (dq_freq.hip's kScanChunk)
constexpr int kMaxChunks = 4096;
// The byte copy.  A cell shorter than kWaveBytes is copied by the lane that owns its row; one of
// kWaveBytes .. kSplitBytes - 1 by the 64 lanes of that wave; a longer one is cut into pieces of
// kSplitBytes that workgroups of their own copy (dq_take_pieces_kernel), so that its length does
// not serialise the launch behind one wave.  (Chosen as DESIGN.md §3 "Take: rows as tables" says.)
// (DQ_TAKE_WAVE_BYTES / DQ_TAKE_SPLIT_BYTES: the sweep's variant builds, tools/bench_take.py.)
#ifndef DQ_TAKE_WAVE_BYTES
#define DQ_TAKE_WAVE_BYTES 16
#endif
#ifndef DQ_TAKE_SPLIT_BYTES
#define DQ_TAKE_SPLIT_BYTES 8192
#endif
constexpr int64_t kWaveBytes = DQ_TAKE_WAVE_BYTES;
constexpr int64_t kSplitBytes = DQ_TAKE_SPLIT_BYTES;
static_assert(kWaveBytes >= 16 && kWaveBytes < kSplitBytes && kSplitBytes >= 4096, "take: byte-copy thresholds");
// Cells of kSplitBytes or more in one output column: their bytes sum to at most INT32_MAX, so a
// list of this capacity that overflows belongs to an output that is refused anyway.
constexpr int64_t kMaxSplitCells = 0x7fffffffll / kSplitBytes + 2;

// ---------------------------------------------------------------- a column as the kernels see it
// One chunk, its slice already applied to the pointers where a byte address can carry it: values =
// the first row's cell (fixed width), the bitmap's base (bool), the heap's base (utf8); offsets =
// the first row's entry (utf8).  Bit buffers keep the slice in bit_offset.
struct Chunk {
  const uint8_t* validity;  // nullptr: every row is valid
  const uint8_t* values;
  const int32_t* offsets;
  int64_t bit_offset;
};

// A piece of a long cell (dq_take_pieces_kernel): bytes [start, start + kSplitBytes) of output row
// `row`.  (The length pass lists the long cells in the same record: start = the cell's length.)
struct Piece {
  int64_t row;
  int64_t start;
};

// The chunk holding global row `idx`: the c with prefix[c] <= idx < prefix[c + 1], for an idx in
// [0, prefix[n_chunks]) and prefix the exclusive running sum of the chunks' rows (n_chunks + 1
// entries, ascending; empty chunks repeat a value and are never the answer).
template <typename P>
DQ_HD inline int find_chunk(const P& prefix, int n_chunks, int64_t idx) {
  int lo = 0, hi = n_chunks;  // prefix[lo] <= idx < prefix[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= idx) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- byte-copy addressing
// The widest unit both addresses allow: 16 bytes when source and destination are congruent mod 16,
// 4 when congruent mod 4, else 1.
DQ_HD inline int copy_unit(uintptr_t src, uintptr_t dst) {
  const uintptr_t x = src ^ dst;
  return (x & 15u) == 0u ? 16 : (x & 3u) == 0u ? 4 : 1;
}

// n < 16 bytes at cell offset `off`, by one lane: 4-byte units where the (common) alignment allows,
// bytes otherwise.
template <typename Op>
DQ_HD inline void copy_ends(uintptr_t dst, int unit, int64_t off, int64_t n, Op& op) {
  while (n > 0) {
    if (unit >= 4 && ((dst + (uintptr_t)off) & 3u) == 0u && n >= 4) {
      op(off, 4);
      off += 4;
      n -= 4;
    } else {
      op(off, 1);
      off += 1;
      n -= 1;
    }
  }
}

// The share of lane `lane` of `n_lanes` in the copy of the cell src[0, len) -> dst[0, len):
// op(offset, width) for every access it makes, width 16, 4 or 1, each one inside [0, len), aligned
// to its width at both addresses, the accesses of all lanes covering every byte exactly once.
// Whole units go round the lanes (consecutive lanes, consecutive units); the bytes before the first
// whole unit are lane 0's, those after the last the last lane's.
template <typename Op>
DQ_HD inline void copy_plan(uintptr_t src, uintptr_t dst, int64_t len, int lane, int n_lanes, Op& op) {
  if (len <= 0) return;
  const int unit = copy_unit(src, dst);
  int64_t head = (int64_t)((uintptr_t)unit - (dst & (uintptr_t)(unit - 1))) & (unit - 1);
  if (head > len) head = len;
  const int64_t units = (len - head) / unit;
  const int64_t tail_at = head + units * unit;
  if (lane == 0) copy_ends(dst, unit, 0, head, op);
  for (int64_t u = lane; u < units; u += n_lanes) op(head + u * unit, unit);
  if (lane == n_lanes - 1) copy_ends(dst, unit, tail_at, len - tail_at, op);
}

}  // namespace take

#if defined(__HIPCC__)
// dq_take.hip
hipError_t launch_take_map(const int64_t* d_rows, int64_t m, const int64_t* d_prefix, int n_chunks, int32_t* d_chunk,
                           int64_t* d_local, unsigned long long* d_status, hipStream_t stream);
hipError_t launch_take_fixed(const take::Chunk* d_chunks, int width, bool aligned16, const int32_t* d_chunk,
                             const int64_t* d_local, int64_t m, void* d_dst, hipStream_t stream);
hipError_t launch_take_bits(const take::Chunk* d_chunks, bool validity, const int32_t* d_chunk, const int64_t* d_local,
                            int64_t m, uint64_t* d_dst, hipStream_t stream);
hipError_t launch_take_len(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local, int64_t m,
                           unsigned long long* d_len, take::Piece* d_split, unsigned long long* d_n_split,
                           hipStream_t stream);
hipError_t launch_take_offsets(const unsigned long long* d_scan, int64_t m, int32_t* d_offsets, hipStream_t stream);
hipError_t launch_take_bytes(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local, int64_t m,
                             const unsigned long long* d_scan, uint8_t* d_dst, hipStream_t stream);
hipError_t launch_take_pieces(const take::Chunk* d_chunks, const int32_t* d_chunk, const int64_t* d_local,
                              const take::Piece* d_pieces, int64_t n_pieces, const unsigned long long* d_scan,
                              uint8_t* d_dst, hipStream_t stream);
#endif

}  // namespace dq
