// dq_take_api.inc -- the dq_take_* family (include/deequ_amd.h "take"): the rows of chunked
// device-resident columns named by global row indices, as new Arrow buffers the caller owns.
// Included by dq_api.cpp (fail, DQ_HIP, DevBuf, dq_ctx, type_size, valid_type).  dq_take_create
// validates the indices and maps them to (chunk, local row) in a pass that reads only the index
// array (dq_take.hip: dq_take_map_kernel); dq_take_layout sizes one column's output (for utf8: the
// length pass and the 64-bit scan) and dq_take_gather writes it.

struct dq_take {
  int device = 0;
  int64_t m = 0, total = 0, n_null = 0;
  std::vector<int64_t> chunk_rows;
  DevBuf d_prefix, d_status, d_chunk, d_local;
  // the column dq_take_layout was last called for
  bool have_layout = false;
  int32_t type = 0;
  int64_t values_bytes = 0, validity_bytes = 0, offsets_bytes = 0, n_pieces = 0;
  bool aligned16 = false;
  std::vector<take::Chunk> chunks;
  DevBuf d_chunks, d_scan, d_sums, d_split, d_n_split, d_pieces;
};

extern "C" dq_status dq_take_create(dq_ctx* ctx, const int64_t* d_rows, int64_t m, const int64_t* chunk_rows,
                                    int n_chunks, dq_take** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !chunk_rows || m < 0 || (m > 0 && !d_rows) || n_chunks < 1)
    return fail(DQ_ERR_INVALID, "dq_take_create: bad argument (a context, m >= 0 indices, at least one chunk)");
  if (n_chunks > take::kMaxChunks)
    return fail(DQ_ERR_UNSUPPORTED, "dq_take_create: " + std::to_string(n_chunks) + " chunks; at most " +
                                        std::to_string(take::kMaxChunks) + " are taken from (concatenate some first)");
  std::unique_ptr<dq_take> t(new dq_take());
  t->device = ctx->device;
  t->m = m;
  t->chunk_rows.assign(chunk_rows, chunk_rows + n_chunks);
  std::vector<int64_t> prefix((size_t)n_chunks + 1, 0);
  for (int c = 0; c < n_chunks; ++c) {
    if (chunk_rows[c] < 0 || chunk_rows[c] > INT64_MAX - prefix[c])
      return fail(DQ_ERR_INVALID, "dq_take_create: chunk " + std::to_string(c) + " has a negative or overflowing row count");
    prefix[c + 1] = prefix[c] + chunk_rows[c];
  }
  t->total = prefix[n_chunks];
  if (m > 0) {
    DQ_HIP(hipSetDevice(ctx->device));
    DQ_TRY(t->d_prefix.ensure(prefix.size() * 8));
    DQ_TRY(t->d_status.ensure(16));
    DQ_TRY(t->d_chunk.ensure((size_t)m * 4));
    DQ_TRY(t->d_local.ensure((size_t)m * 8));
    unsigned long long status[2] = {0ull, ~0ull};
    DQ_HIP(hipMemcpy(t->d_prefix.ptr, prefix.data(), prefix.size() * 8, hipMemcpyHostToDevice));
    DQ_HIP(hipMemcpy(t->d_status.ptr, status, 16, hipMemcpyHostToDevice));
    DQ_HIP(launch_take_map(d_rows, m, static_cast<const int64_t*>(t->d_prefix.ptr), n_chunks,
                           static_cast<int32_t*>(t->d_chunk.ptr), static_cast<int64_t*>(t->d_local.ptr),
                           static_cast<unsigned long long*>(t->d_status.ptr), nullptr));
    DQ_HIP(hipMemcpy(status, t->d_status.ptr, 16, hipMemcpyDeviceToHost));
    if (status[1] != ~0ull) {
      if (status[1] >= (unsigned long long)m) return fail(DQ_ERR_DEVICE, "dq_take_create: corrupt validation result");
      int64_t value = 0;
      DQ_HIP(hipMemcpy(&value, d_rows + status[1], 8, hipMemcpyDeviceToHost));
      return fail(DQ_ERR_INVALID, "dq_take_create: rows[" + std::to_string(status[1]) + "] = " + std::to_string(value) +
                                      " is outside [-1, " + std::to_string(t->total) + ") (-1: no row)");
    }
    if (status[0] > (unsigned long long)m) return fail(DQ_ERR_DEVICE, "dq_take_create: corrupt validation result");
    t->n_null = (int64_t)status[0];
  }
  *out = t.release();
  return DQ_OK;
}

extern "C" dq_status dq_take_info(dq_take* t, int64_t* n_null_rows) {
  if (!t || !n_null_rows) return fail(DQ_ERR_INVALID, "dq_take_info: NULL argument");
  *n_null_rows = t->n_null;
  return DQ_OK;
}

extern "C" dq_status dq_take_destroy(dq_take* t) {
  delete t;
  return DQ_OK;
}

// The chunks of one column as the kernels address them (no device work).
static dq_status take_stage_chunks(dq_take* t, const dq_column* cols, std::vector<take::Chunk>* out, bool* any_validity,
                                   bool* aligned16) {
  const int n_chunks = (int)t->chunk_rows.size();
  const int32_t type = cols[0].type;
  if (!valid_type(type)) return fail(DQ_ERR_INVALID, "dq_take_layout: unknown column type");
  const size_t w = (size_t)type_size(type);
  out->assign((size_t)n_chunks, take::Chunk{nullptr, nullptr, nullptr, 0});
  *any_validity = false;
  *aligned16 = true;
  for (int c = 0; c < n_chunks; ++c) {
    const dq_column& col = cols[c];
    const std::string name = "dq_take_layout: chunk " + std::to_string(c);
    if (col.type != type) return fail(DQ_ERR_INVALID, name + " has another type than chunk 0");
    if (!(col.flags & DQ_COL_DEVICE))
      return fail(DQ_ERR_INVALID, name + " is host-resident: take reads DQ_COL_DEVICE columns in place");
    if (col.length != t->chunk_rows[c] || col.offset < 0)
      return fail(DQ_ERR_INVALID, name + " has " + std::to_string(col.length) + " rows, the handle was created for " +
                                      std::to_string(t->chunk_rows[c]));
    take::Chunk& k = (*out)[c];
    k.validity = col.validity;
    k.bit_offset = col.offset;
    if (col.validity) *any_validity = true;
    if (col.length == 0) continue;  // (no index maps to it: its pointers are never read)
    if (type == DQ_T_UTF8) {
      if (!col.offsets || (reinterpret_cast<uintptr_t>(col.offsets) & 3u))
        return fail(DQ_ERR_INVALID, name + ": a utf8 column without (4-byte aligned) offsets");
      k.offsets = col.offsets + col.offset;
      k.values = static_cast<const uint8_t*>(col.values);  // (NULL only when every cell is empty)
    } else {
      if (!col.values) return fail(DQ_ERR_INVALID, name + ": a column without values");
      k.values = static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w;
      const uintptr_t a = reinterpret_cast<uintptr_t>(k.values);
      if (w > 1 && (a & (std::min<size_t>(w, 8) - 1)))
        return fail(DQ_ERR_INVALID, name + ": values are not aligned to their width");
      if (a & 15u) *aligned16 = false;
    }
  }
  return DQ_OK;
}

extern "C" dq_status dq_take_layout(dq_take* t, const dq_column* chunks, int32_t* type, int64_t* values_bytes,
                                    int64_t* validity_bytes, int64_t* offsets_bytes) {
  if (!t || !chunks || !type || !values_bytes || !validity_bytes || !offsets_bytes)
    return fail(DQ_ERR_INVALID, "dq_take_layout: NULL argument");
  t->have_layout = false;
  bool any_validity = false;
  DQ_TRY(take_stage_chunks(t, chunks, &t->chunks, &any_validity, &t->aligned16));
  const int32_t ty = chunks[0].type;
  const int64_t m = t->m, words = (m + 63) / 64;
  t->type = ty;
  t->validity_bytes = (m > 0 && (any_validity || t->n_null > 0)) ? words * 8 : 0;
  t->offsets_bytes = ty == DQ_T_UTF8 ? (m + 1) * 4 : 0;
  t->values_bytes = ty == DQ_T_UTF8 ? 0 : ty == DQ_T_BOOL ? words * 8 : m * type_size(ty);
  t->n_pieces = 0;
  if (m > 0) {
    DQ_HIP(hipSetDevice(t->device));
    DQ_TRY(t->d_chunks.ensure(t->chunks.size() * sizeof(take::Chunk)));
    DQ_HIP(hipMemcpy(t->d_chunks.ptr, t->chunks.data(), t->chunks.size() * sizeof(take::Chunk), hipMemcpyHostToDevice));
  }
  if (ty == DQ_T_UTF8 && m > 0) {
    DQ_TRY(t->d_scan.ensure((size_t)(m + 1) * 8));
    DQ_TRY(t->d_sums.ensure(((size_t)(m + 1) / take::kScanTile + 2) * 8));
    DQ_TRY(t->d_split.ensure((size_t)take::kMaxSplitCells * sizeof(take::Piece)));
    DQ_TRY(t->d_n_split.ensure(8));
    unsigned long long* scan = static_cast<unsigned long long*>(t->d_scan.ptr);
    DQ_HIP(hipMemsetAsync(t->d_n_split.ptr, 0, 8, nullptr));
    DQ_HIP(launch_take_len(static_cast<const take::Chunk*>(t->d_chunks.ptr), static_cast<const int32_t*>(t->d_chunk.ptr),
                           static_cast<const int64_t*>(t->d_local.ptr), m, scan,
                           static_cast<take::Piece*>(t->d_split.ptr),
                           static_cast<unsigned long long*>(t->d_n_split.ptr), nullptr));
    DQ_HIP(scan_exclusive_u64(scan, (uint64_t)m + 1, static_cast<unsigned long long*>(t->d_sums.ptr), nullptr));
    unsigned long long total = 0, n_split = 0;
    DQ_HIP(hipMemcpy(&total, scan + m, 8, hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(&n_split, t->d_n_split.ptr, 8, hipMemcpyDeviceToHost));
    if (total > 0x7fffffffull)
      return fail(DQ_ERR_SPACE, "dq_take_layout: the gathered strings hold " + std::to_string(total) +
                                    " bytes; a utf8 output's int32 offsets reach 2147483647 (take fewer rows at a time)");
    if (n_split > (unsigned long long)take::kMaxSplitCells) return fail(DQ_ERR_DEVICE, "dq_take_layout: corrupt cell list");
    if (n_split > 0) {
      std::vector<take::Piece> cells((size_t)n_split), pieces;
      DQ_HIP(hipMemcpy(cells.data(), t->d_split.ptr, cells.size() * sizeof(take::Piece), hipMemcpyDeviceToHost));
      for (const take::Piece& c : cells) {
        if (c.row < 0 || c.row >= m || c.start < take::kSplitBytes || c.start > (int64_t)total)
          return fail(DQ_ERR_DEVICE, "dq_take_layout: corrupt cell list");
        for (int64_t at = 0; at < c.start; at += take::kSplitBytes) pieces.push_back(take::Piece{c.row, at});
      }
      DQ_TRY(t->d_pieces.ensure(pieces.size() * sizeof(take::Piece)));
      DQ_HIP(hipMemcpy(t->d_pieces.ptr, pieces.data(), pieces.size() * sizeof(take::Piece), hipMemcpyHostToDevice));
      t->n_pieces = (int64_t)pieces.size();
    }
    t->values_bytes = (int64_t)total;
  }
  *type = ty;
  *values_bytes = t->values_bytes;
  *validity_bytes = t->validity_bytes;
  *offsets_bytes = t->offsets_bytes;
  t->have_layout = true;
  return DQ_OK;
}

extern "C" dq_status dq_take_gather(dq_take* t, const dq_column* chunks, void* values, void* validity, void* offsets) {
  if (!t || !chunks) return fail(DQ_ERR_INVALID, "dq_take_gather: NULL argument");
  if (!t->have_layout) return fail(DQ_ERR_STATE, "dq_take_gather before dq_take_layout (or after one that failed)");
  std::vector<take::Chunk> now;
  bool any_validity = false, aligned16 = false;
  DQ_TRY(take_stage_chunks(t, chunks, &now, &any_validity, &aligned16));
  if (chunks[0].type != t->type || now.size() != t->chunks.size() ||
      (!now.empty() && std::memcmp(now.data(), t->chunks.data(), now.size() * sizeof(take::Chunk)) != 0))
    return fail(DQ_ERR_STATE, "dq_take_gather: not the column dq_take_layout was last called for");
  if ((t->values_bytes > 0 && !values) || (t->validity_bytes > 0 && !validity) || (t->offsets_bytes > 0 && !offsets))
    return fail(DQ_ERR_INVALID, "dq_take_gather: an output buffer is NULL");
  const int64_t m = t->m;
  const uintptr_t va = reinterpret_cast<uintptr_t>(values);
  const size_t w = (size_t)type_size(t->type);
  if ((reinterpret_cast<uintptr_t>(validity) & 7u) || (reinterpret_cast<uintptr_t>(offsets) & 3u) ||
      (t->type == DQ_T_BOOL && (va & 7u)) || (w > 1 && (va & (std::min<size_t>(w, 8) - 1))))
    return fail(DQ_ERR_INVALID, "dq_take_gather: an output buffer is not aligned (bit buffers: 8 bytes; values: their width)");
  DQ_HIP(hipSetDevice(t->device));
  if (m == 0) {
    if (t->offsets_bytes > 0) DQ_HIP(hipMemset(offsets, 0, 4));
    return DQ_OK;
  }
  const take::Chunk* d_chunks = static_cast<const take::Chunk*>(t->d_chunks.ptr);
  const int32_t* d_chunk = static_cast<const int32_t*>(t->d_chunk.ptr);
  const int64_t* d_local = static_cast<const int64_t*>(t->d_local.ptr);
  if (t->type == DQ_T_UTF8) {
    const unsigned long long* scan = static_cast<const unsigned long long*>(t->d_scan.ptr);
    DQ_HIP(launch_take_offsets(scan, m, static_cast<int32_t*>(offsets), nullptr));
    if (t->values_bytes > 0) {
      DQ_HIP(launch_take_bytes(d_chunks, d_chunk, d_local, m, scan, static_cast<uint8_t*>(values), nullptr));
      DQ_HIP(launch_take_pieces(d_chunks, d_chunk, d_local, static_cast<const take::Piece*>(t->d_pieces.ptr), t->n_pieces,
                                scan, static_cast<uint8_t*>(values), nullptr));
    }
  } else if (t->type == DQ_T_BOOL) {
    DQ_HIP(launch_take_bits(d_chunks, false, d_chunk, d_local, m, static_cast<uint64_t*>(values), nullptr));
  } else {
    DQ_HIP(launch_take_fixed(d_chunks, (int)w, t->aligned16 && (va & 15u) == 0u, d_chunk, d_local, m, values, nullptr));
  }
  if (t->validity_bytes > 0)
    DQ_HIP(launch_take_bits(d_chunks, true, d_chunk, d_local, m, static_cast<uint64_t*>(validity), nullptr));
  DQ_HIP(hipStreamSynchronize(nullptr));
  return DQ_OK;
}

// The tiling constants of dq_take.h (tests derive their shapes from them).
extern "C" dq_status dq_diag_take_constants(int64_t* out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  out[0] = take::kRowsPerBlock;
  out[1] = take::kScanTile;
  out[2] = take::kWaveBytes;
  out[3] = take::kSplitBytes;
  return DQ_OK;
}
