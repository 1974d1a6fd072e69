// dq_corrmat_api.inc -- the dq_corrmat_* family (include/deequ_amd.h): every pairwise Correlation
// state of up to 64 numeric columns in one pass over each batch (dq_corrmat.hip), the pairs the
// matrix sums do not answer from the pair kernel (launch_corr, dq_pair.hip) over the same batch and
// mask -- or, where a sum of finite values overflowed, from Spark's per-row update (launch_corrmat_rows).  Included at the end of dq_api.cpp (shares DevBuf, Stager, prepare_column,
// validate_predicate, ProgramTables, StreamPool, fail, DQ_HIP) and holds the host mirror
// dq_diag_corrmat_host (include/deequ_amd_diag.h).

struct dq_corrmat : Stager {
  dq_ctx* ctx = nullptr;
  std::vector<bool> col_used;
  std::vector<int32_t> sel;  // the matrix's columns, in the caller's order
  int k = 0;
  int64_t n_pairs = 0;
  int n_cu = 0;
  // the optional `where`: one program, laid out as a plan's (ProgramTables)
  bool has_where = false;
  PredProgram prog{0, 0};
  int n_matches = 0;
  uint32_t lds = 0;
  bool cast = false;
  std::vector<DevColumn> h_cols;
  std::vector<uint32_t> h_flags;
  int64_t fallback_pairs = 0;
  DevBuf d_progs, d_insns, d_pool, d_match, d_dfas, d_cols, d_words, d_match_words, d_masks, d_sel, d_partials, d_batch,
      d_running, d_flags, d_tasks, d_fb_index, d_fb_acc, d_fb_part;

  ~dq_corrmat() {
    if (stream) StreamPool::get().release(ctx ? ctx->device : 0, stream);
    stream = nullptr;
  }
};

extern "C" dq_status dq_corrmat_create(dq_ctx* ctx, const int32_t* column_types, int n_columns, const int32_t* columns,
                                       int n_selected, const dq_predicate* where, dq_corrmat** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !column_types || !columns || n_columns <= 0) return fail(DQ_ERR_INVALID, "NULL argument");
  if (n_selected < 1) return fail(DQ_ERR_INVALID, "dq_corrmat_create: no column selected");
  if (n_selected > kCorrmatMaxCols)
    return fail(DQ_ERR_UNSUPPORTED, "correlation matrix of " + std::to_string(n_selected) + " columns: one matrix holds at most " +
                                        std::to_string(kCorrmatMaxCols) + " (cut the columns into blocks)");
  for (int c = 0; c < n_columns; ++c)
    if (!valid_type(column_types[c])) return fail(DQ_ERR_INVALID, "invalid column type");
  std::unique_ptr<dq_corrmat> m(new dq_corrmat());
  m->ctx = ctx;
  m->col_types.assign(column_types, column_types + n_columns);
  m->col_used.assign(n_columns, false);
  m->k = n_selected;
  m->n_pairs = corrmat_pairs(n_selected);
  for (int i = 0; i < n_selected; ++i) {
    const int c = columns[i];
    if (c < 0 || c >= n_columns) return fail(DQ_ERR_INVALID, "dq_corrmat_create: column out of range");
    if (!is_numeric(column_types[c]))
      return fail(DQ_ERR_INVALID, "dq_corrmat_create: column " + std::to_string(c) + " is not numeric");
    for (int j = 0; j < i; ++j)
      if (columns[j] == c) return fail(DQ_ERR_INVALID, "dq_corrmat_create: column " + std::to_string(c) + " is selected twice");
    m->sel.push_back(c);
    m->col_used[c] = true;
  }
  std::vector<MatchTask> tasks;
  std::vector<std::string> keys;
  std::vector<uint32_t> offsets;
  std::vector<uint8_t> images;
  ProgramTables tables{{}, {}, false, tasks, keys, offsets, images, m->lds};
  if (where && where->code && where->n_insns > 0) {
    Program prog;
    DQ_TRY(validate_predicate(*where, column_types, n_columns, &prog));
    for (int c : prog.columns) m->col_used[c] = true;
    m->prog = tables.add(prog);
    m->has_where = true;
  }
  m->n_matches = (int)tasks.size();
  m->cast = tables.cast;
  DQ_HIP(hipSetDevice(ctx->device));
  DQ_HIP(hipDeviceGetAttribute(&m->n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  hipError_t e = StreamPool::get().acquire(ctx->device, &m->stream);
  if (e != hipSuccess) return fail(DQ_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  std::string pool = tables.pool;
  pool.append(8, '\0');
  auto upload = [&](DevBuf& buf, const void* src, size_t bytes) -> dq_status {
    if (bytes == 0) return DQ_OK;
    DQ_TRY(buf.ensure(bytes));
    DQ_HIP(hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
    return DQ_OK;
  };
  if (m->has_where) {
    DQ_TRY(upload(m->d_progs, &m->prog, sizeof(PredProgram)));
    DQ_TRY(upload(m->d_insns, tables.insns.data(), tables.insns.size() * sizeof(PredInsn)));
    DQ_TRY(upload(m->d_pool, pool.data(), pool.size()));
    DQ_TRY(upload(m->d_match, tasks.data(), tasks.size() * sizeof(MatchTask)));
    DQ_TRY(upload(m->d_dfas, images.data(), images.size()));
    DQ_TRY(m->d_masks.ensure(sizeof(DevMask)));
  }
  DQ_TRY(upload(m->d_sel, m->sel.data(), m->sel.size() * sizeof(int32_t)));
  DQ_TRY(m->d_cols.ensure(n_columns * sizeof(DevColumn)));
  DQ_TRY(m->d_batch.ensure((size_t)m->n_pairs * sizeof(CorrAcc)));
  DQ_TRY(m->d_running.ensure((size_t)m->n_pairs * sizeof(CorrAcc)));
  DQ_TRY(m->d_flags.ensure((size_t)(m->n_pairs + m->k) * sizeof(uint32_t)));
  DQ_HIP(hipMemset(m->d_running.ptr, 0, (size_t)m->n_pairs * sizeof(CorrAcc)));
  m->h_flags.resize((size_t)(m->n_pairs + m->k));
  m->resize_stage(n_columns);
  m->h_cols.resize(n_columns);
  *out = m.release();
  return DQ_OK;
}

extern "C" dq_status dq_corrmat_consume(dq_corrmat* m, const dq_column* columns, int n_columns, int64_t n_rows) {
  if (!m) return fail(DQ_ERR_INVALID, "corrmat is NULL");
  if (n_columns != (int)m->col_types.size()) return fail(DQ_ERR_INVALID, "column count differs from the plan");
  if (n_rows < 0) return fail(DQ_ERR_INVALID, "negative n_rows");
  if (n_rows == 0) return DQ_OK;
  if (!columns) return fail(DQ_ERR_INVALID, "columns is NULL");
  if (n_rows > (int64_t)1 << 40) return fail(DQ_ERR_INVALID, "batch too large (split it)");
  DQ_HIP(hipSetDevice(m->ctx->device));
  for (int c = 0; c < n_columns; ++c) {
    std::memset(&m->h_cols[c], 0, sizeof(DevColumn));
    if (m->col_used[c]) DQ_TRY(prepare_column(m, c, columns[c], n_rows, &m->h_cols[c]));
  }
  DQ_HIP(hipMemcpyAsync(m->d_cols.ptr, m->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice, m->stream));
  const DevColumn* dcols = static_cast<const DevColumn*>(m->d_cols.ptr);
  const uint64_t* where_t = nullptr;
  if (m->has_where) {  // the filter's TRUE / NOT NULL planes: launch_predicates, as a plan's masks
    const int64_t wpm = ((n_rows + 63) >> 6) + 1;
    if (m->n_matches > 0) {
      DQ_TRY(m->d_match_words.ensure((size_t)wpm * m->n_matches * sizeof(uint64_t)));
      DQ_HIP(launch_match_mask(static_cast<const MatchTask*>(m->d_match.ptr), m->n_matches, dcols,
                               static_cast<const uint8_t*>(m->d_dfas.ptr), m->lds, n_rows,
                               static_cast<uint64_t*>(m->d_match_words.ptr), wpm, m->stream));
    }
    DQ_TRY(m->d_words.ensure((size_t)wpm * 2 * sizeof(uint64_t)));
    DQ_HIP(launch_predicates(static_cast<const PredProgram*>(m->d_progs.ptr), 1, static_cast<const PredInsn*>(m->d_insns.ptr),
                             static_cast<const uint8_t*>(m->d_pool.ptr), dcols, n_rows, static_cast<uint64_t*>(m->d_words.ptr),
                             wpm, m->cast, m->stream, static_cast<const uint64_t*>(m->d_match_words.ptr)));
    where_t = static_cast<const uint64_t*>(m->d_words.ptr);
    const DevMask mask{where_t, where_t + wpm};
    DQ_HIP(hipMemcpyAsync(m->d_masks.ptr, &mask, sizeof(mask), hipMemcpyHostToDevice, m->stream));
  }
  bool masked = m->has_where;
  for (int c : m->sel) masked = masked || m->h_cols[c].validity != nullptr;

  // slabs -> row ranges: two resident workgroups per CU (one in the masked form)
  const int64_t n_slabs = corrmat_n_slabs(n_rows);
  const int64_t max_ranges = (int64_t)std::max(1, m->n_cu) * (masked ? 1 : 2);
  const int64_t per = corrmat_slabs_per_range(n_slabs, max_ranges);
  const int64_t n_ranges = (n_slabs + per - 1) / per;
  const size_t n_flags = (size_t)(m->n_pairs + m->k);
  DQ_TRY(m->d_partials.ensure((size_t)n_ranges * (size_t)m->n_pairs * sizeof(CorrAcc)));
  uint32_t* d_flags = static_cast<uint32_t*>(m->d_flags.ptr);
  DQ_HIP(hipMemsetAsync(d_flags, 0, n_flags * sizeof(uint32_t), m->stream));
  CorrAcc* d_batch = static_cast<CorrAcc*>(m->d_batch.ptr);
  DQ_HIP(launch_corrmat(masked, dcols, static_cast<const int32_t*>(m->d_sel.ptr), m->k, where_t, n_rows, per, (int)n_ranges,
                        static_cast<CorrAcc*>(m->d_partials.ptr), d_batch, d_flags, d_flags + m->n_pairs, m->stream));
  // the one readback of a batch: a flag per pair and per column
  DQ_HIP(hipMemcpyAsync(m->h_flags.data(), d_flags, n_flags * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  DQ_HIP(hipStreamSynchronize(m->stream));
  // fall-backs: the pair kernel's tasks first, then the tasks of Spark's per-row update (a sum of
  // finite values that was not finite: the pair kernel's Sxx - Sx² / n would be Inf - Inf there)
  std::vector<CorrTask> tasks, row_tasks;
  std::vector<int64_t> row_pairs;
  std::vector<int32_t> fb_index((size_t)m->n_pairs, -1);
  for (int i = 0; i < m->k; ++i)
    for (int j = i; j < m->k; ++j) {
      const int64_t p = corrmat_pair_index(i, j, m->k);
      const bool bad = m->h_flags[(size_t)(m->n_pairs + i)] || m->h_flags[(size_t)(m->n_pairs + j)];
      const CorrTask t{m->sel[i], m->sel[j], m->has_where ? 0 : -1, 0};
      if (!bad && (m->h_flags[(size_t)p] & kCorrmatNonFinite)) {
        row_pairs.push_back(p);
        row_tasks.push_back(t);
      } else if (bad || m->h_flags[(size_t)p]) {
        fb_index[(size_t)p] = (int32_t)tasks.size();
        tasks.push_back(t);
      }
    }
  const int n_pk = (int)tasks.size(), n_rw = (int)row_tasks.size(), n_fb = n_pk + n_rw;
  for (int t = 0; t < n_rw; ++t) fb_index[(size_t)row_pairs[(size_t)t]] = n_pk + t;
  tasks.insert(tasks.end(), row_tasks.begin(), row_tasks.end());
  const int32_t* d_fb_index = nullptr;
  if (n_fb > 0) {  // over the same columns and mask
    auto blocks = [&](int n) {
      const int64_t b = std::max<int64_t>(1, std::max<int64_t>(256, 8 * (int64_t)m->n_cu) / std::max(1, n));
      return std::min<int64_t>(b, (n_rows + kBlock - 1) / kBlock);
    };
    const int64_t bpt = blocks(n_pk), bpt_rows = blocks(n_rw);
    DQ_TRY(m->d_tasks.ensure((size_t)n_fb * sizeof(CorrTask)));
    DQ_TRY(m->d_fb_index.ensure((size_t)m->n_pairs * sizeof(int32_t)));
    DQ_TRY(m->d_fb_acc.ensure((size_t)n_fb * sizeof(CorrAcc)));
    DQ_TRY(m->d_fb_part.ensure(((size_t)n_pk * (size_t)bpt + (size_t)n_rw * (size_t)bpt_rows) * sizeof(CorrAcc)));
    DQ_HIP(hipMemcpyAsync(m->d_tasks.ptr, tasks.data(), (size_t)n_fb * sizeof(CorrTask), hipMemcpyHostToDevice, m->stream));
    DQ_HIP(hipMemcpyAsync(m->d_fb_index.ptr, fb_index.data(), (size_t)m->n_pairs * sizeof(int32_t), hipMemcpyHostToDevice,
                          m->stream));
    DQ_HIP(hipMemsetAsync(m->d_fb_acc.ptr, 0, (size_t)n_fb * sizeof(CorrAcc), m->stream));
    const CorrTask* d_tasks = static_cast<const CorrTask*>(m->d_tasks.ptr);
    const DevMask* d_masks = static_cast<const DevMask*>(m->d_masks.ptr);
    CorrAcc* d_part = static_cast<CorrAcc*>(m->d_fb_part.ptr);
    CorrAcc* d_acc = static_cast<CorrAcc*>(m->d_fb_acc.ptr);
    DQ_HIP(launch_corr(d_tasks, n_pk, dcols, d_masks, n_rows, (int)bpt, d_part, d_acc, m->stream));
    DQ_HIP(launch_corrmat_rows(d_tasks + n_pk, n_rw, dcols, d_masks, n_rows, (int)bpt_rows, d_part + (size_t)n_pk * (size_t)bpt,
                               d_acc + n_pk, m->stream));
    d_fb_index = static_cast<const int32_t*>(m->d_fb_index.ptr);
    m->fallback_pairs += n_fb;
  }
  DQ_HIP(launch_corrmat_combine(d_batch, static_cast<const CorrAcc*>(m->d_fb_acc.ptr), d_fb_index, m->n_pairs,
                                static_cast<CorrAcc*>(m->d_running.ptr), m->stream));
  DQ_HIP(hipStreamSynchronize(m->stream));  // (the host vectors above are read by the copies)
  m->host_tmp.clear();
  return DQ_OK;
}

extern "C" dq_status dq_corrmat_finish(dq_corrmat* m, double* states, int64_t* fallback_pairs) {
  if (!m || !states) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(m->ctx->device));
  std::vector<CorrAcc> acc((size_t)m->n_pairs);
  DQ_HIP(hipMemcpyAsync(acc.data(), m->d_running.ptr, acc.size() * sizeof(CorrAcc), hipMemcpyDeviceToHost, m->stream));
  DQ_HIP(hipStreamSynchronize(m->stream));
  for (size_t p = 0; p < acc.size(); ++p) {
    const CorrAcc& a = acc[p];
    double* o = states + 6 * p;
    if (a.n == 0.0) {
      o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0;
    } else {
      o[0] = a.n, o[1] = a.xavg, o[2] = a.yavg, o[3] = a.ck, o[4] = a.xmk, o[5] = a.ymk;
    }
  }
  if (fallback_pairs) *fallback_pairs = m->fallback_pairs;
  return DQ_OK;
}

extern "C" dq_status dq_corrmat_reset(dq_corrmat* m) {
  if (!m) return fail(DQ_ERR_INVALID, "corrmat is NULL");
  DQ_HIP(hipSetDevice(m->ctx->device));
  DQ_HIP(hipMemsetAsync(m->d_running.ptr, 0, (size_t)m->n_pairs * sizeof(CorrAcc), m->stream));
  DQ_HIP(hipStreamSynchronize(m->stream));
  m->fallback_pairs = 0;
  return DQ_OK;
}

extern "C" dq_status dq_corrmat_destroy(dq_corrmat* m) {
  delete m;
  return DQ_OK;
}

extern "C" dq_status dq_diag_corrmat_host(const double* const* columns, const uint8_t* const* valid, const uint8_t* where,
                                          int32_t n_selected, int64_t n_rows, int64_t max_ranges, double* states,
                                          uint8_t* flags) {
  if (!columns || !states || !flags || n_selected < 1 || n_selected > kCorrmatMaxCols || n_rows < 0)
    return fail(DQ_ERR_INVALID, "dq_diag_corrmat_host: bad argument");
  for (int i = 0; i < n_selected; ++i)
    if (!columns[i] && n_rows > 0) return fail(DQ_ERR_INVALID, "dq_diag_corrmat_host: a column is NULL");
  corrmat_host(columns, valid, where, n_selected, n_rows, max_ranges, states, flags);
  return DQ_OK;
}
