// dq_quantile_api.inc -- the dq_aq_* family (include/deequ_amd.h): ApproxQuantile's runner.  Included
// by dq_api.cpp (fail, DQ_HIP, DevBuf, dq_ctx).  Per batch: the radix select's passes for every
// (column, relativeError) pair in one launch each (dq_quantile.hip), then each pair's keys at its
// target ranks come to the host, become the batch summary and are merged into the running digest
// (dq_quantile.cpp), in arrival order.

namespace dq {
hipError_t launch_aq_pass(const aq::DevAqPair* d_pairs, aq::DevAqWork* d_work, int n_pairs, int64_t n_rows, int pass,
                          hipStream_t stream);
}  // namespace dq

struct AqColumnState {
  int32_t column = 0;
  double eps = 0;
  aq::Digest running;
  DevBuf values, validity;
};

struct dq_aq {
  int device = 0;
  std::vector<int32_t> types;
  std::vector<AqColumnState> cols;
  int passes = 0;  // the most passes a batch can take for the smallest relativeError of the run
  DevBuf d_pairs, d_work;
};

static std::string aq_num(double v) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.15g", v);
  return buf;
}

extern "C" dq_status dq_aq_supported(double relative_error) {
  if (!(relative_error >= 0.0 && relative_error <= 1.0))
    return fail(DQ_ERR_INVALID, "ApproxQuantile: relativeError " + aq_num(relative_error) + " is outside [0, 1]");
  if (relative_error == 0.0)
    return fail(DQ_ERR_UNSUPPORTED,
                "ApproxQuantile(relativeError=0.0): an exact quantile needs a full sort of the column; the GPU "
                "select is bound to relativeError >= " + aq_num(aq::kMinRelativeError));
  if (relative_error < aq::kMinRelativeError)
    return fail(DQ_ERR_UNSUPPORTED, "ApproxQuantile(relativeError=" + aq_num(relative_error) +
                                        "): the GPU select keeps at most " + std::to_string(aq::kMaxRanks) +
                                        " target ranks per batch and is bound to relativeError >= " +
                                        aq_num(aq::kMinRelativeError));
  return DQ_OK;
}

extern "C" dq_status dq_aq_create(dq_ctx* ctx, const dq_aq_column* columns, int n, const int32_t* column_types,
                                  int n_columns, dq_aq** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !columns || !column_types || n < 1 || n > 1024 || n_columns < 1)
    return fail(DQ_ERR_INVALID, "dq_aq_create: bad argument (1 to 1024 digests)");
  std::unique_ptr<dq_aq> s(new dq_aq());
  s->device = ctx->device;
  s->types.assign(column_types, column_types + n_columns);
  s->cols.resize(n);
  for (int i = 0; i < n; ++i) {
    AqColumnState& c = s->cols[i];
    c.column = columns[i].column;
    c.eps = columns[i].relative_error;
    if (c.column < 0 || c.column >= n_columns) return fail(DQ_ERR_INVALID, "dq_aq_create: column out of range");
    if (!is_numeric(column_types[c.column]))
      return fail(DQ_ERR_INVALID, "dq_aq_create: column " + std::to_string(c.column) + " is not numeric");
    DQ_TRY(dq_aq_supported(c.eps));
    c.running = aq::Digest(c.eps);
    const int ranks = (int)std::min<double>(aq::kMaxRanks, std::floor(2.0 / c.eps) + 2.0);
    s->passes = std::max(s->passes, aq::max_passes(ranks));
  }
  *out = s.release();
  return DQ_OK;
}

extern "C" dq_status dq_aq_destroy(dq_aq* s) {
  delete s;
  return DQ_OK;
}

extern "C" dq_status dq_aq_consume(dq_aq* s, const dq_column* columns, int n_columns, int64_t n_rows) {
  if (!s || !columns || n_columns != (int)s->types.size() || n_rows < 0)
    return fail(DQ_ERR_INVALID, "dq_aq_consume: bad argument");
  if (n_rows > 0x7fffffff)
    return fail(DQ_ERR_UNSUPPORTED, "ApproxQuantile: a batch of " + std::to_string(n_rows) +
                                        " rows; the GPU select counts rows and gaps in 32 bits and is bound to "
                                        "2147483647 rows per batch");
  if (n_rows == 0) return DQ_OK;
  DQ_HIP(hipSetDevice(s->device));
  const int n = (int)s->cols.size();
  std::vector<aq::DevAqPair> dp(n);
  for (int i = 0; i < n; ++i) {
    AqColumnState& c = s->cols[i];
    const dq_column& col = columns[c.column];
    if (col.type != s->types[c.column]) return fail(DQ_ERR_INVALID, "dq_aq_consume: column type differs from the schema");
    if (col.length < n_rows || col.offset < 0) return fail(DQ_ERR_INVALID, "dq_aq_consume: column shorter than the batch");
    if (!col.values) return fail(DQ_ERR_INVALID, "dq_aq_consume: values is NULL");
    const size_t w = (size_t)type_size(col.type);
    aq::DevAqPair& d = dp[i];
    memset(&d, 0, sizeof(d));
    if (col.flags & DQ_COL_DEVICE) {
      d.values = static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w;
      d.validity = col.validity;
      d.bit_offset = col.offset;
    } else {
      DQ_TRY(c.values.ensure((size_t)n_rows * w));
      DQ_HIP(hipMemcpy(c.values.ptr, static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w,
                       (size_t)n_rows * w, hipMemcpyHostToDevice));
      d.values = c.values.ptr;
      d.bit_offset = col.offset & 7;
      if (col.validity) {
        const size_t first = (size_t)(col.offset >> 3), bytes = (size_t)((d.bit_offset + n_rows + 7) >> 3);
        DQ_TRY(c.validity.ensure(bytes));
        DQ_HIP(hipMemcpy(c.validity.ptr, col.validity + first, bytes, hipMemcpyHostToDevice));
        d.validity = static_cast<const uint8_t*>(c.validity.ptr);
      }
    }
    d.type = col.type;
    d.eps = c.eps;
  }
  DQ_TRY(s->d_pairs.ensure(sizeof(aq::DevAqPair) * (size_t)n));
  DQ_TRY(s->d_work.ensure(sizeof(aq::DevAqWork) * (size_t)n));
  DQ_HIP(hipMemcpy(s->d_pairs.ptr, dp.data(), sizeof(aq::DevAqPair) * (size_t)n, hipMemcpyHostToDevice));
  DQ_HIP(hipMemsetAsync(s->d_work.ptr, 0, sizeof(aq::DevAqWork) * (size_t)n, nullptr));
  const aq::DevAqPair* d_pairs = static_cast<const aq::DevAqPair*>(s->d_pairs.ptr);
  aq::DevAqWork* d_work = static_cast<aq::DevAqWork*>(s->d_work.ptr);
  for (int pass = 0; pass < s->passes; ++pass) DQ_HIP(launch_aq_pass(d_pairs, d_work, n, n_rows, pass, nullptr));
  DQ_HIP(hipStreamSynchronize(nullptr));
  std::vector<uint64_t> keys;
  for (int i = 0; i < n; ++i) {
    AqColumnState& c = s->cols[i];
    aq::DevAqState st;
    DQ_HIP(hipMemcpy(&st, &d_work[i].st, sizeof(st), hipMemcpyDeviceToHost));
    if (st.error || !st.done || st.n < 0 || st.n > n_rows || st.m < 0 || st.m > aq::kMaxRanks ||
        (st.n > 0 && st.m != aq::batch_ranks(st.n, aq::batch_gap(c.eps, st.n))))
      return fail(DQ_ERR_DEVICE, "ApproxQuantile: the select did not finish (error " + std::to_string(st.error) +
                                     ", " + std::to_string(st.m) + " target ranks)");
    if (st.n == 0) continue;  // every row NULL: an empty side of the merge
    keys.resize((size_t)st.m);
    DQ_HIP(hipMemcpy(keys.data(), d_work[i].keys, (size_t)st.m * 8, hipMemcpyDeviceToHost));
    const aq::Digest batch = aq::Digest::from_batch(c.eps, st.n, keys.data(), st.m);
    if (!c.running.merge(batch)) return fail(DQ_ERR_STATE, "ApproxQuantile: digests of different relativeError");
  }
  return DQ_OK;
}

extern "C" dq_status dq_aq_finish(dq_aq* s, int64_t* sizes, int n) {
  if (!s || !sizes || n != (int)s->cols.size()) return fail(DQ_ERR_INVALID, "dq_aq_finish: bad argument");
  for (int i = 0; i < n; ++i) {
    if (!s->cols[i].running.fits_int32())
      return fail(DQ_ERR_UNSUPPORTED, "ApproxQuantile: a digest entry's g or delta does not fit the serialised form's Int");
    sizes[i] = s->cols[i].running.serialised_bytes();
  }
  return DQ_OK;
}

extern "C" dq_status dq_aq_export(dq_aq* s, int i, void* out, int64_t capacity, int64_t* required) {
  if (!s || i < 0 || i >= (int)s->cols.size()) return fail(DQ_ERR_INVALID, "dq_aq_export: bad argument");
  const aq::Digest& d = s->cols[i].running;
  const int64_t need = d.serialised_bytes();
  if (required) *required = need;
  if (!out || capacity < need) return fail(DQ_ERR_SPACE, "dq_aq_export: the buffer is too small");
  if (!d.fits_int32())
    return fail(DQ_ERR_UNSUPPORTED, "ApproxQuantile: a digest entry's g or delta does not fit the serialised form's Int");
  d.serialise(static_cast<uint8_t*>(out));
  return DQ_OK;
}
