// dq_rows_api.inc -- row-level outcomes of the scan analyzers (include/deequ_amd.h "row-level
// outcomes") over the predicate interpreter, the match-mask kernel and dq_rows.hip.
// Included at the end of dq_api.cpp (shares DevBuf, Stager, prepare_column, check_op,
// validate_predicate, ProgramTables, fail, DQ_HIP).

struct dq_rows : Stager {
  dq_ctx* ctx = nullptr;
  std::vector<bool> col_used;
  // One outcome per op: what it counts (Completeness: its column's validity; Compliance: program
  // `cond`'s TRUE plane; PatternMatch: match task `match`'s mask) and the program of its `where`.
  struct Outcome {
    int kind, column, cond, match, where;
  };
  std::vector<Outcome> outs;
  // the programs' tables, laid out as a plan's (ProgramTables); PatternMatch's images lie in
  // d_dfas next to those of the programs' LIKE / RLIKE, its tasks among theirs
  std::vector<PredProgram> progs;
  int n_matches = 0;
  uint32_t lds = 0;
  bool cast = false;
  std::vector<DevColumn> h_cols;
  DevBuf d_progs, d_insns, d_pool, d_match, d_dfas, d_cols, d_words, d_match_words;

  ~dq_rows() {
    if (stream) StreamPool::get().release(ctx ? ctx->device : 0, stream);
    stream = nullptr;
  }
};

extern "C" dq_status dq_rows_create(dq_ctx* ctx, const dq_op* ops, int n_ops, const int32_t* column_types,
                                    int n_columns, dq_rows** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !ops || !column_types || n_ops <= 0 || n_columns <= 0) return fail(DQ_ERR_INVALID, "NULL argument");
  for (int c = 0; c < n_columns; ++c)
    if (!valid_type(column_types[c])) return fail(DQ_ERR_INVALID, "invalid column type");
  std::unique_ptr<dq_rows> r(new dq_rows());
  r->ctx = ctx;
  r->col_types.assign(column_types, column_types + n_columns);
  r->col_used.assign(n_columns, false);
  std::vector<MatchTask> tasks;
  std::vector<std::string> keys;
  std::vector<uint32_t> offsets;
  std::vector<uint8_t> images;
  ProgramTables tables{{}, {}, false, tasks, keys, offsets, images, r->lds};
  auto add_program = [&](const dq_predicate& p, int* index) -> dq_status {
    Program prog;
    DQ_TRY(validate_predicate(p, column_types, n_columns, &prog));
    for (int c : prog.columns) r->col_used[c] = true;
    *index = (int)r->progs.size();
    r->progs.push_back(tables.add(prog));
    return DQ_OK;
  };
  for (int i = 0; i < n_ops; ++i) {
    const dq_op& op = ops[i];
    if (op.kind != DQ_OP_COMPLETENESS && op.kind != DQ_OP_COMPLIANCE && op.kind != DQ_OP_PATTERN_MATCH)
      return fail(DQ_ERR_INVALID, "op kind " + std::to_string(op.kind) + " has no row-level outcome (Completeness, "
                                  "Compliance and PatternMatch have)");
    regex::Dfa dfa;
    DQ_TRY(check_op(op, column_types, n_columns, &dfa));
    dq_rows::Outcome o{op.kind, op.column, -1, -1, -1};
    if (op.kind == DQ_OP_COMPLIANCE) {
      DQ_TRY(add_program(op.predicate, &o.cond));
    } else {
      r->col_used[op.column] = true;
    }
    if (op.kind == DQ_OP_PATTERN_MATCH) {  // the scan's DFA (regex::compile), walked by the match-mask kernel
      const std::vector<uint8_t> image = dfa.image();
      o.match = (int)tasks.size();
      tasks.push_back(MatchTask{op.column, (uint32_t)images.size()});
      images.insert(images.end(), image.begin(), image.end());
      r->lds = std::max(r->lds, (uint32_t)image.size() - regex::kRegexHeaderBytes);
    }
    if (op.where.code && op.where.n_insns > 0) DQ_TRY(add_program(op.where, &o.where));
    r->outs.push_back(o);
  }
  r->n_matches = (int)tasks.size();
  r->cast = tables.cast;
  DQ_HIP(hipSetDevice(ctx->device));
  hipError_t e = StreamPool::get().acquire(ctx->device, &r->stream);
  if (e != hipSuccess) return fail(DQ_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  std::string pool = tables.pool;
  pool.append(8, '\0');
  auto upload = [&](DevBuf& buf, const void* src, size_t bytes) -> dq_status {
    if (bytes == 0) return DQ_OK;
    DQ_TRY(buf.ensure(bytes));
    DQ_HIP(hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
    return DQ_OK;
  };
  DQ_TRY(upload(r->d_progs, r->progs.data(), r->progs.size() * sizeof(PredProgram)));
  DQ_TRY(upload(r->d_insns, tables.insns.data(), tables.insns.size() * sizeof(PredInsn)));
  DQ_TRY(upload(r->d_pool, pool.data(), pool.size()));
  DQ_TRY(upload(r->d_match, tasks.data(), tasks.size() * sizeof(MatchTask)));
  DQ_TRY(upload(r->d_dfas, images.data(), images.size()));
  DQ_TRY(r->d_cols.ensure(n_columns * sizeof(DevColumn)));
  r->resize_stage(n_columns);
  r->h_cols.resize(n_columns);
  *out = r.release();
  return DQ_OK;
}

extern "C" dq_status dq_rows_evaluate(dq_rows* r, const dq_column* columns, int n_columns, int64_t n_rows,
                                      int64_t out_bit_offset, uint64_t* const* d_value, uint64_t* const* d_valid) {
  if (!r) return fail(DQ_ERR_INVALID, "rows is NULL");
  if (n_columns != (int)r->col_types.size()) return fail(DQ_ERR_INVALID, "column count differs from the plan");
  if (n_rows < 0 || out_bit_offset < 0) return fail(DQ_ERR_INVALID, "negative n_rows or out_bit_offset");
  if (n_rows == 0) return DQ_OK;
  if (!columns || !d_value || !d_valid) return fail(DQ_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < r->outs.size(); ++i)
    if (!d_value[i] || !d_valid[i]) return fail(DQ_ERR_INVALID, "NULL output bitmap");
  DQ_HIP(hipSetDevice(r->ctx->device));
  for (int c = 0; c < n_columns; ++c) {
    std::memset(&r->h_cols[c], 0, sizeof(DevColumn));
    if (r->col_used[c]) DQ_TRY(prepare_column(r, c, columns[c], n_rows, &r->h_cols[c]));
  }
  DQ_HIP(hipMemcpyAsync(r->d_cols.ptr, r->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                        r->stream));
  const DevColumn* dcols = static_cast<const DevColumn*>(r->d_cols.ptr);
  const int64_t wpm = ((n_rows + 63) >> 6) + 1;  // words per plane
  const int n_progs = (int)r->progs.size();
  if (r->n_matches > 0) {
    DQ_TRY(r->d_match_words.ensure((size_t)wpm * r->n_matches * sizeof(uint64_t)));
    DQ_HIP(launch_match_mask(static_cast<const MatchTask*>(r->d_match.ptr), r->n_matches, dcols,
                             static_cast<const uint8_t*>(r->d_dfas.ptr), r->lds, n_rows,
                             static_cast<uint64_t*>(r->d_match_words.ptr), wpm, r->stream));
  }
  if (n_progs > 0) {
    DQ_TRY(r->d_words.ensure((size_t)wpm * 2 * n_progs * sizeof(uint64_t)));
    DQ_HIP(launch_predicates(static_cast<const PredProgram*>(r->d_progs.ptr), n_progs,
                             static_cast<const PredInsn*>(r->d_insns.ptr), static_cast<const uint8_t*>(r->d_pool.ptr),
                             dcols, n_rows, static_cast<uint64_t*>(r->d_words.ptr), wpm, r->cast, r->stream,
                             static_cast<const uint64_t*>(r->d_match_words.ptr)));
  }
  const uint64_t* words = static_cast<const uint64_t*>(r->d_words.ptr);
  const uint64_t* match_words = static_cast<const uint64_t*>(r->d_match_words.ptr);
  for (size_t i = 0; i < r->outs.size(); ++i) {
    const dq_rows::Outcome& o = r->outs[i];
    const uint8_t* cond_bytes = nullptr;
    const uint64_t* cond_words = nullptr;
    if (o.kind == DQ_OP_COMPLETENESS) cond_bytes = r->h_cols[o.column].validity;  // (nullptr: every row is valid)
    else if (o.kind == DQ_OP_COMPLIANCE) cond_words = words + (int64_t)(2 * o.cond) * wpm;
    else cond_words = match_words + (int64_t)o.match * wpm;
    const uint64_t* sel = o.where >= 0 ? words + (int64_t)(2 * o.where) * wpm : nullptr;
    DQ_HIP(launch_rows_combine(cond_bytes, cond_words, sel, n_rows, out_bit_offset, d_value[i], d_valid[i], r->stream));
  }
  DQ_HIP(hipStreamSynchronize(r->stream));
  r->host_tmp.clear();
  return DQ_OK;
}

extern "C" dq_status dq_rows_destroy(dq_rows* r) {
  delete r;
  return DQ_OK;
}

extern "C" dq_status dq_rows_select(dq_ctx* ctx, const uint64_t* d_value, const uint64_t* d_valid, int64_t n_rows,
                                    int which, int64_t* d_out, int64_t capacity, int64_t* n_out) {
  if (!ctx || !n_out) return fail(DQ_ERR_INVALID, "NULL argument");
  *n_out = 0;
  if (n_rows < 0 || capacity < 0) return fail(DQ_ERR_INVALID, "negative n_rows or capacity");
  if (which <= 0 || (which & ~(DQ_ROWS_FALSE | DQ_ROWS_TRUE | DQ_ROWS_NULL)))
    return fail(DQ_ERR_INVALID, "which is an OR of DQ_ROWS_FALSE, DQ_ROWS_TRUE, DQ_ROWS_NULL");
  if (n_rows == 0) return DQ_OK;
  if (!d_value || !d_valid || (capacity > 0 && !d_out)) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(ctx->device));
  DevBuf counts, sums;  // (released after the stream they were used on is idle: declared before its lease)
  struct Lease {  // a pooled stream for the length of the call
    int device;
    hipStream_t s = nullptr;
    ~Lease() { StreamPool::get().release(device, s); }
  } lease{ctx->device};
  hipError_t e = StreamPool::get().acquire(ctx->device, &lease.s);
  if (e != hipSuccess) return fail(DQ_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  const uint64_t n = (uint64_t)((n_rows + 63) >> 6) + 1;  // the words' counts and the total
  DQ_TRY(counts.ensure(n * sizeof(unsigned long long)));
  DQ_TRY(sums.ensure(((n + 4095) / 4096 + 1) * sizeof(unsigned long long)));
  unsigned long long* c = static_cast<unsigned long long*>(counts.ptr);
  DQ_HIP(launch_rows_select_count(d_value, d_valid, n_rows, which, c, lease.s));
  DQ_HIP(scan_exclusive_u64(c, n, static_cast<unsigned long long*>(sums.ptr), lease.s));
  unsigned long long total = 0;
  DQ_HIP(hipMemcpyAsync(&total, c + (n - 1), sizeof(total), hipMemcpyDeviceToHost, lease.s));
  DQ_HIP(hipStreamSynchronize(lease.s));
  *n_out = (int64_t)total;
  if ((int64_t)total > capacity) return fail(DQ_ERR_SPACE, "dq_rows_select: capacity is below the selected rows");
  if (total == 0) return DQ_OK;
  DQ_HIP(launch_rows_select_scatter(d_value, d_valid, n_rows, which, c, d_out, capacity, lease.s));
  DQ_HIP(hipStreamSynchronize(lease.s));
  return DQ_OK;
}
