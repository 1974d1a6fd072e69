// dq_schema_api.inc -- the dq_schema_* family (include/deequ_amd.h): RowLevelSchemaValidator's
// runner.  Included by dq_api.cpp (fail, DQ_HIP, DevBuf, dq_ctx).  dq_schema_validate evaluates the
// schema over one batch (dq_schema.hip: evaluate, combine, scan, select) and sizes every output
// column; dq_schema_gather then writes one output column into buffers the caller allocated, so the
// rows land in memory their owner manages and are written once.

namespace dq {
hipError_t launch_schema_eval(const schema::DevDef* d_defs, int n_defs, const schema::DevCol* d_cols,
                              const uint8_t* d_dfas, uint32_t lds_bytes, int64_t n_rows, int blocks_per_def,
                              uint64_t* d_false, uint64_t* d_null, uint8_t* d_scratch, uint32_t* d_unsupported,
                              hipStream_t stream);
hipError_t launch_schema_combine(const uint64_t* d_false, const uint64_t* d_null, int n_defs, int64_t n_rows,
                                 uint64_t* d_valid_bm, uint64_t* d_invalid_bm, uint32_t* d_cnt_valid,
                                 uint32_t* d_cnt_invalid, hipStream_t stream);
hipError_t launch_schema_select(const uint64_t* d_valid_bm, const uint64_t* d_invalid_bm, const uint32_t* d_pre_valid,
                                const uint32_t* d_pre_invalid, int64_t n_rows, int32_t* d_sel_valid,
                                int32_t* d_sel_invalid, hipStream_t stream);
hipError_t launch_schema_gather_fixed(const void* d_src, int width, const int32_t* d_sel, int64_t m, void* d_dst,
                                      hipStream_t stream);
hipError_t launch_schema_gather_bits(const uint8_t* d_src, int64_t bit_offset, const int32_t* d_sel, int64_t m,
                                     uint64_t* d_dst, hipStream_t stream);
hipError_t launch_schema_gather_len(const schema::DevCol& col, const int32_t* d_sel, int64_t m, uint32_t* d_len,
                                    hipStream_t stream);
hipError_t launch_schema_gather_bytes(const schema::DevCol& col, const int32_t* d_sel, int64_t m,
                                      const int32_t* d_new_offs, uint8_t* d_dst, hipStream_t stream);
}  // namespace dq

struct SchemaColumnBufs {
  DevBuf values, validity, offsets;  // a host column's slice, uploaded
  DevBuf new_offs[2];                // utf8: the offsets of the valid / invalid output (count + 1 entries)
  int64_t out_bytes[2] = {0, 0};     // utf8: the heap bytes of each output
};

struct dq_schema {
  int device = 0;
  std::vector<int32_t> types;
  std::vector<schema::DevDef> defs;
  std::vector<int32_t> cast_def;     // per column: the definition that decides its cast (the last), or -1
  std::vector<uint8_t> dfas;         // the compiled patterns' images, back to back (16-byte aligned)
  uint32_t lds_bytes = 0;
  int64_t scratch_row_bytes = 0;     // bytes of parsed values per row, over all definitions
  // the last batch
  bool have_batch = false, declined = false;
  int64_t n_rows = 0, count[2] = {0, 0};
  std::vector<schema::DevCol> cols;
  std::vector<SchemaColumnBufs> bufs;
  std::vector<int64_t> scratch_off;  // per definition, for the last batch's row count
  DevBuf d_defs, d_cols, d_dfas, d_false, d_null, d_scratch, d_flags, d_bm[2], d_cnt[2], d_sums, d_sel[2], d_len;
};

static std::string schema_def_name(int i, const dq_schema_def& d) {
  return "definition " + std::to_string(i) + " (column " + std::to_string(d.column) + ")";
}

// The plan: every definition checked and compiled into *s (no device work).
static dq_status schema_plan(const dq_schema_def* defs, int n_defs, const int32_t* column_types, int n_columns,
                             dq_schema* s) {
  if ((n_defs > 0 && !defs) || !column_types || n_defs < 0 || n_defs > 4096 || n_columns < 1)
    return fail(DQ_ERR_INVALID, "dq_schema_create: bad argument (at most 4096 definitions, at least one column)");
  s->types.assign(column_types, column_types + n_columns);
  for (int c = 0; c < n_columns; ++c)
    if (!valid_type(column_types[c])) return fail(DQ_ERR_INVALID, "dq_schema_create: unknown column type");
  for (int c = 0; c < n_columns; ++c)  // (the gathers move 1- to 8-byte values: DESIGN.md §7)
    if (is_decimal(column_types[c]))
      return fail(DQ_ERR_UNSUPPORTED, "column " + std::to_string(c) + " is a " + decimal_name(column_types[c]) +
                                          " column: decimal columns in the validator's input are not on the GPU path");
  s->cast_def.assign((size_t)n_columns, -1);
  s->defs.resize((size_t)n_defs);
  for (int i = 0; i < n_defs; ++i) {
    const dq_schema_def& d = defs[i];
    schema::DevDef& k = s->defs[i];
    memset(&k, 0, sizeof(k));
    if (d.column < 0 || d.column >= n_columns)
      return fail(DQ_ERR_INVALID, "dq_schema_create: " + schema_def_name(i, d) + ": column out of range");
    if (d.kind == DQ_SCHEMA_DECIMAL && (d.precision < 1 || d.precision > 38 || d.scale < 0 || d.scale > d.precision))
      return fail(DQ_ERR_INVALID, "dq_schema_create: " + schema_def_name(i, d) + ": DecimalType(" +
                                      std::to_string(d.precision) + ", " + std::to_string(d.scale) +
                                      ") needs 1 <= precision <= 38 and 0 <= scale <= precision");
    if (d.kind == DQ_SCHEMA_TIMESTAMP)
      return fail(DQ_ERR_UNSUPPORTED, schema_def_name(i, d) +
                                          ": timestamp columns are not validated on the GPU (Spark 2.2's "
                                          "unix_timestamp is a lenient SimpleDateFormat)");
    if (d.kind != DQ_SCHEMA_STRING && d.kind != DQ_SCHEMA_INT && d.kind != DQ_SCHEMA_DECIMAL)
      return fail(DQ_ERR_INVALID, "dq_schema_create: " + schema_def_name(i, d) + ": unknown kind");
    if (column_types[d.column] != DQ_T_UTF8)
      return fail(DQ_ERR_UNSUPPORTED, schema_def_name(i, d) + ": the schema is enforced on string columns only");
    k.column = d.column;
    k.flags = (d.flags & DQ_SCHEMA_NOT_NULL) ? schema::DF_NOT_NULL : 0;
    if (d.kind != DQ_SCHEMA_DECIMAL) {
      if (((d.flags & DQ_SCHEMA_HAS_MIN) && (d.min_value < INT32_MIN || d.min_value > INT32_MAX)) ||
          ((d.flags & DQ_SCHEMA_HAS_MAX) && (d.max_value < INT32_MIN || d.max_value > INT32_MAX)))
        return fail(DQ_ERR_INVALID, "dq_schema_create: " + schema_def_name(i, d) + ": a bound outside 32 bits");
      if (d.flags & DQ_SCHEMA_HAS_MIN) k.flags |= schema::DF_MIN, k.lo = (int32_t)d.min_value;
      if (d.flags & DQ_SCHEMA_HAS_MAX) k.flags |= schema::DF_MAX, k.hi = (int32_t)d.max_value;
    }
    if (d.kind == DQ_SCHEMA_INT) {
      k.kind = schema::DEF_INT;
      s->scratch_row_bytes += 4;
    } else if (d.kind == DQ_SCHEMA_DECIMAL) {
      if (d.precision > schema::kMaxDecimalPrecision)
        return fail(DQ_ERR_UNSUPPORTED, schema_def_name(i, d) + ": decimal precision " + std::to_string(d.precision) +
                                            " exceeds " + std::to_string(schema::kMaxDecimalPrecision) +
                                            " (unscaled values are 64-bit on the GPU)");
      k.kind = schema::DEF_DECIMAL;
      k.precision = d.precision;
      k.scale = d.scale;
      s->scratch_row_bytes += 8;
    } else {
      k.kind = schema::DEF_STRING;
      if (d.flags & DQ_SCHEMA_HAS_PATTERN) {
        if (!d.pattern || d.pattern_len < 0)
          return fail(DQ_ERR_INVALID, "dq_schema_create: " + schema_def_name(i, d) + ": pattern is NULL");
        regex::Dfa dfa;
        std::string err;
        if (!regex::compile(d.pattern, d.pattern_len, &dfa, &err))
          return fail(DQ_ERR_UNSUPPORTED, schema_def_name(i, d) + ": matches: " + err);
        const std::vector<uint8_t> img = dfa.image();
        k.flags |= schema::DF_MATCH;
        k.dfa_off = (uint32_t)s->dfas.size();
        s->dfas.insert(s->dfas.end(), img.begin(), img.end());
        s->lds_bytes = std::max<uint32_t>(s->lds_bytes, (uint32_t)img.size() - regex::kRegexHeaderBytes);
      }
    }
    s->cast_def[d.column] = d.kind == DQ_SCHEMA_STRING ? -1 : i;  // castExpressions.toMap: the last one wins
  }
  return DQ_OK;
}

extern "C" dq_status dq_schema_supported(const dq_schema_def* defs, int n_defs, const int32_t* column_types,
                                         int n_columns) {
  dq_schema s;
  return schema_plan(defs, n_defs, column_types, n_columns, &s);
}

extern "C" dq_status dq_schema_create(dq_ctx* ctx, const dq_schema_def* defs, int n_defs, const int32_t* column_types,
                                      int n_columns, dq_schema** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx) return fail(DQ_ERR_INVALID, "dq_schema_create: ctx is NULL");
  std::unique_ptr<dq_schema> s(new dq_schema());
  s->device = ctx->device;
  DQ_TRY(schema_plan(defs, n_defs, column_types, n_columns, s.get()));
  *out = s.release();
  return DQ_OK;
}

extern "C" dq_status dq_schema_destroy(dq_schema* s) {
  delete s;
  return DQ_OK;
}

// One input column as the kernels address it; a host column's slice is uploaded first.
static dq_status schema_stage_column(const dq_column& col, int64_t n, SchemaColumnBufs& b, schema::DevCol* out) {
  schema::DevCol d;
  memset(&d, 0, sizeof(d));
  d.type = col.type;
  if (col.length < n || col.offset < 0) return fail(DQ_ERR_INVALID, "dq_schema_validate: column shorter than the batch");
  if (n == 0) {
    *out = d;
    return DQ_OK;
  }
  const size_t w = (size_t)type_size(col.type);
  if (col.type == DQ_T_UTF8 ? !col.offsets : !col.values)
    return fail(DQ_ERR_INVALID, "dq_schema_validate: a column without values / offsets");
  if (col.flags & DQ_COL_DEVICE) {
    d.validity = col.validity;
    d.bit_offset = col.offset;
    d.values = w ? static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w : static_cast<const uint8_t*>(col.values);
    d.offsets = col.offsets ? col.offsets + col.offset : nullptr;
    *out = d;
    return DQ_OK;
  }
  d.bit_offset = col.offset & 7;
  const size_t first_byte = (size_t)(col.offset >> 3), bit_bytes = (size_t)((d.bit_offset + n + 7) >> 3);
  if (col.validity) {
    DQ_TRY(b.validity.ensure(bit_bytes));
    DQ_HIP(hipMemcpy(b.validity.ptr, col.validity + first_byte, bit_bytes, hipMemcpyHostToDevice));
    d.validity = static_cast<const uint8_t*>(b.validity.ptr);
  }
  if (col.type == DQ_T_UTF8) {
    const int32_t* offs = col.offsets + col.offset;
    const int64_t first = offs[0], last = offs[n];
    if (first < 0 || last < first) return fail(DQ_ERR_INVALID, "dq_schema_validate: utf8 offsets out of order");
    if (last > first && !col.values) return fail(DQ_ERR_INVALID, "dq_schema_validate: a utf8 column without values");
    DQ_TRY(b.offsets.ensure((size_t)(n + 1) * 4));
    DQ_HIP(hipMemcpy(b.offsets.ptr, offs, (size_t)(n + 1) * 4, hipMemcpyHostToDevice));
    DQ_TRY(b.values.ensure((size_t)(last - first)));
    if (last > first)
      DQ_HIP(hipMemcpy(b.values.ptr, static_cast<const uint8_t*>(col.values) + first, (size_t)(last - first),
                       hipMemcpyHostToDevice));
    d.offsets = static_cast<const int32_t*>(b.offsets.ptr);
    d.values = b.values.ptr;
    d.heap_base = (int32_t)first;
  } else if (col.type == DQ_T_BOOL) {
    DQ_TRY(b.values.ensure(bit_bytes));
    DQ_HIP(hipMemcpy(b.values.ptr, static_cast<const uint8_t*>(col.values) + first_byte, bit_bytes, hipMemcpyHostToDevice));
    d.values = b.values.ptr;
  } else {
    DQ_TRY(b.values.ensure((size_t)n * w));
    DQ_HIP(hipMemcpy(b.values.ptr, static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w, (size_t)n * w,
                     hipMemcpyHostToDevice));
    d.values = b.values.ptr;
  }
  *out = d;
  return DQ_OK;
}

extern "C" dq_status dq_schema_validate(dq_schema* s, const dq_column* columns, int n_columns, int64_t n_rows,
                                        int64_t* num_valid, int64_t* num_invalid, int32_t* def_flags) {
  if (!s || !columns || n_columns != (int)s->types.size() || n_rows < 0 || !num_valid || !num_invalid)
    return fail(DQ_ERR_INVALID, "dq_schema_validate: bad argument");
  if (n_rows > 0x7fffffff - 64) return fail(DQ_ERR_UNSUPPORTED, "dq_schema_validate: more than 2^31 - 65 rows in one batch");
  DQ_HIP(hipSetDevice(s->device));
  s->have_batch = false;
  s->declined = false;
  const int n_defs = (int)s->defs.size();
  const int64_t n = n_rows, n_words = (n + 63) / 64;
  if (def_flags)
    for (int i = 0; i < n_defs; ++i) def_flags[i] = 0;
  s->cols.assign((size_t)n_columns, schema::DevCol{});
  s->bufs.resize((size_t)n_columns);
  for (int c = 0; c < n_columns; ++c) {
    if (columns[c].type != s->types[c]) return fail(DQ_ERR_INVALID, "dq_schema_validate: column type differs from the schema");
    DQ_TRY(schema_stage_column(columns[c], n, s->bufs[c], &s->cols[c]));
    s->bufs[c].out_bytes[0] = s->bufs[c].out_bytes[1] = 0;
  }
  s->n_rows = n;
  s->count[0] = s->count[1] = 0;
  if (n > 0) {
    // the parsed columns: definition i's dense values from scratch_off[i] (8-byte aligned)
    s->scratch_off.assign((size_t)n_defs, 0);
    int64_t scratch = 0;
    for (int i = 0; i < n_defs; ++i) {
      s->defs[i].scratch_off = s->scratch_off[i] = scratch;
      const int64_t w = s->defs[i].kind == schema::DEF_INT ? 4 : s->defs[i].kind == schema::DEF_DECIMAL ? 8 : 0;
      scratch += (n * w + 7) & ~(int64_t)7;
    }
    DQ_TRY(s->d_scratch.ensure((size_t)scratch));
    DQ_TRY(s->d_defs.ensure(sizeof(schema::DevDef) * (size_t)std::max(1, n_defs)));
    DQ_TRY(s->d_cols.ensure(sizeof(schema::DevCol) * (size_t)n_columns));
    DQ_TRY(s->d_dfas.ensure(s->dfas.size()));
    DQ_TRY(s->d_false.ensure((size_t)std::max(1, n_defs) * (size_t)n_words * 8));
    DQ_TRY(s->d_null.ensure((size_t)std::max(1, n_defs) * (size_t)n_words * 8));
    DQ_TRY(s->d_flags.ensure((size_t)std::max(1, n_defs) * 4));
    for (int k = 0; k < 2; ++k) {
      DQ_TRY(s->d_bm[k].ensure((size_t)n_words * 8));
      DQ_TRY(s->d_cnt[k].ensure((size_t)(n_words + 1) * 4));
    }
    DQ_TRY(s->d_sums.ensure(((size_t)(n + 1) / 4096 + 2) * 4));
    if (n_defs > 0) DQ_HIP(hipMemcpy(s->d_defs.ptr, s->defs.data(), sizeof(schema::DevDef) * (size_t)n_defs, hipMemcpyHostToDevice));
    DQ_HIP(hipMemcpy(s->d_cols.ptr, s->cols.data(), sizeof(schema::DevCol) * (size_t)n_columns, hipMemcpyHostToDevice));
    if (!s->dfas.empty()) DQ_HIP(hipMemcpy(s->d_dfas.ptr, s->dfas.data(), s->dfas.size(), hipMemcpyHostToDevice));
    DQ_HIP(hipMemsetAsync(s->d_flags.ptr, 0, (size_t)std::max(1, n_defs) * 4, nullptr));
    hipDeviceProp_t prop;
    DQ_HIP(hipGetDeviceProperties(&prop, s->device));
    const int64_t want = (n_words + kBlock / 64 - 1) / (kBlock / 64);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)prop.multiProcessorCount * 8));
    uint64_t* d_false = static_cast<uint64_t*>(s->d_false.ptr);
    uint64_t* d_null = static_cast<uint64_t*>(s->d_null.ptr);
    DQ_HIP(launch_schema_eval(static_cast<const schema::DevDef*>(s->d_defs.ptr), n_defs,
                              static_cast<const schema::DevCol*>(s->d_cols.ptr),
                              static_cast<const uint8_t*>(s->d_dfas.ptr), s->lds_bytes, n, blocks, d_false, d_null,
                              static_cast<uint8_t*>(s->d_scratch.ptr), static_cast<uint32_t*>(s->d_flags.ptr), nullptr));
    uint32_t* cnt[2] = {static_cast<uint32_t*>(s->d_cnt[0].ptr), static_cast<uint32_t*>(s->d_cnt[1].ptr)};
    uint64_t* bm[2] = {static_cast<uint64_t*>(s->d_bm[0].ptr), static_cast<uint64_t*>(s->d_bm[1].ptr)};
    DQ_HIP(launch_schema_combine(d_false, d_null, n_defs, n, bm[0], bm[1], cnt[0], cnt[1], nullptr));
    for (int k = 0; k < 2; ++k)
      DQ_HIP(scan_exclusive_u32(cnt[k], (uint64_t)n_words + 1, static_cast<uint32_t*>(s->d_sums.ptr), nullptr));
    std::vector<uint32_t> flags((size_t)std::max(1, n_defs), 0);
    uint32_t totals[2] = {0, 0};
    for (int k = 0; k < 2; ++k) DQ_HIP(hipMemcpy(&totals[k], cnt[k] + n_words, 4, hipMemcpyDeviceToHost));
    DQ_HIP(hipMemcpy(flags.data(), s->d_flags.ptr, (size_t)std::max(1, n_defs) * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n_defs; ++i)
      if (flags[i]) {
        if (def_flags) def_flags[i] = 1;
        if (!s->declined)
          fail(DQ_ERR_UNSUPPORTED, "definition " + std::to_string(i) + " (column " + std::to_string(s->defs[i].column) +
                                       "): a decimal cell holds a non-ASCII byte or an exponent beyond " +
                                       std::to_string(schema::kMaxDecimalExponent) +
                                       "; the GPU cannot judge it as java.math.BigDecimal does");
        s->declined = true;
      }
    if (s->declined) return DQ_ERR_UNSUPPORTED;
    if ((int64_t)totals[0] + (int64_t)totals[1] > n) return fail(DQ_ERR_DEVICE, "dq_schema_validate: corrupt row counts");
    s->count[0] = totals[0];
    s->count[1] = totals[1];
    for (int k = 0; k < 2; ++k) DQ_TRY(s->d_sel[k].ensure((size_t)std::max<int64_t>(1, s->count[k]) * 4));
    DQ_HIP(launch_schema_select(bm[0], bm[1], cnt[0], cnt[1], n, static_cast<int32_t*>(s->d_sel[0].ptr),
                                static_cast<int32_t*>(s->d_sel[1].ptr), nullptr));
  }
  // the utf8 outputs' offsets (and with them their heap sizes)
  for (int c = 0; c < n_columns; ++c) {
    if (s->types[c] != DQ_T_UTF8) continue;
    for (int k = 0; k < 2; ++k) {
      if (k == 0 && s->cast_def[c] >= 0) continue;  // cast: not a string in validRows
      const int64_t m = s->count[k];
      SchemaColumnBufs& b = s->bufs[c];
      DQ_TRY(b.new_offs[k].ensure((size_t)(m + 1) * 4));
      uint32_t* offs = static_cast<uint32_t*>(b.new_offs[k].ptr);
      if (m == 0) {
        DQ_HIP(hipMemsetAsync(offs, 0, 4, nullptr));
        continue;
      }
      DQ_TRY(s->d_sums.ensure(((size_t)(m + 1) / 4096 + 2) * 4));
      DQ_HIP(launch_schema_gather_len(s->cols[c], static_cast<const int32_t*>(s->d_sel[k].ptr), m, offs, nullptr));
      DQ_HIP(scan_exclusive_u32(offs, (uint64_t)m + 1, static_cast<uint32_t*>(s->d_sums.ptr), nullptr));
      uint32_t total = 0;
      DQ_HIP(hipMemcpy(&total, offs + m, 4, hipMemcpyDeviceToHost));
      if (total > 0x7fffffffu) return fail(DQ_ERR_DEVICE, "dq_schema_validate: corrupt output offsets");
      b.out_bytes[k] = total;
    }
  }
  DQ_HIP(hipStreamSynchronize(nullptr));
  *num_valid = s->count[0];
  *num_invalid = s->count[1];
  s->have_batch = true;
  return DQ_OK;
}

static dq_status schema_output_check(dq_schema* s, int which, int column, const char* fn) {
  if (!s || which < 0 || which > 1 || column < 0 || column >= (int)s->types.size())
    return fail(DQ_ERR_INVALID, std::string(fn) + ": bad argument");
  if (!s->have_batch)
    return fail(DQ_ERR_STATE, std::string(fn) + (s->declined ? ": the last batch was declined" : " before dq_schema_validate"));
  return DQ_OK;
}

extern "C" dq_status dq_schema_output_layout(dq_schema* s, int which, int column, int32_t* type, int64_t* values_bytes,
                                             int64_t* validity_bytes, int64_t* offsets_bytes) {
  DQ_TRY(schema_output_check(s, which, column, "dq_schema_output_layout"));
  if (!type || !values_bytes || !validity_bytes || !offsets_bytes)
    return fail(DQ_ERR_INVALID, "dq_schema_output_layout: bad argument");
  const int64_t m = s->count[which];
  const int cd = which == 0 ? s->cast_def[column] : -1;
  int32_t t = s->types[column];
  if (cd >= 0) t = s->defs[cd].kind == schema::DEF_INT ? DQ_T_INT32 : DQ_T_INT64;
  *type = t;
  *offsets_bytes = t == DQ_T_UTF8 ? (m + 1) * 4 : 0;
  *values_bytes = t == DQ_T_UTF8 ? s->bufs[column].out_bytes[which] : t == DQ_T_BOOL ? ((m + 63) / 64) * 8 : m * type_size(t);
  *validity_bytes = (s->n_rows > 0 && s->cols[column].validity) ? ((m + 63) / 64) * 8 : 0;
  return DQ_OK;
}

extern "C" dq_status dq_schema_gather(dq_schema* s, int which, int column, void* values, void* validity, void* offsets) {
  DQ_TRY(schema_output_check(s, which, column, "dq_schema_gather"));
  int32_t t;
  int64_t vb, nb, ob;
  DQ_TRY(dq_schema_output_layout(s, which, column, &t, &vb, &nb, &ob));
  if ((vb > 0 && !values) || (nb > 0 && !validity) || (ob > 0 && !offsets))
    return fail(DQ_ERR_INVALID, "dq_schema_gather: an output buffer is NULL");
  DQ_HIP(hipSetDevice(s->device));
  const int64_t m = s->count[which];
  const int32_t* sel = static_cast<const int32_t*>(s->d_sel[which].ptr);
  const schema::DevCol& col = s->cols[column];
  const int cd = which == 0 ? s->cast_def[column] : -1;
  if (ob > 0)
    DQ_HIP(hipMemcpyAsync(offsets, s->bufs[column].new_offs[which].ptr, (size_t)ob, hipMemcpyDeviceToDevice, nullptr));
  if (m > 0) {
    if (cd >= 0)
      DQ_HIP(launch_schema_gather_fixed(static_cast<const uint8_t*>(s->d_scratch.ptr) + s->scratch_off[cd],
                                        type_size(t), sel, m, values, nullptr));
    else if (t == DQ_T_UTF8)
      DQ_HIP(launch_schema_gather_bytes(col, sel, m, static_cast<const int32_t*>(s->bufs[column].new_offs[which].ptr),
                                        static_cast<uint8_t*>(values), nullptr));
    else if (t == DQ_T_BOOL)
      DQ_HIP(launch_schema_gather_bits(static_cast<const uint8_t*>(col.values), col.bit_offset, sel, m,
                                       static_cast<uint64_t*>(values), nullptr));
    else
      DQ_HIP(launch_schema_gather_fixed(col.values, type_size(t), sel, m, values, nullptr));
    if (nb > 0)
      DQ_HIP(launch_schema_gather_bits(col.validity, col.bit_offset, sel, m, static_cast<uint64_t*>(validity), nullptr));
  }
  DQ_HIP(hipStreamSynchronize(nullptr));
  return DQ_OK;
}

extern "C" dq_status dq_schema_selection(dq_schema* s, int which, int32_t* out, int64_t capacity) {
  DQ_TRY(schema_output_check(s, which, 0, "dq_schema_selection"));
  const int64_t m = s->count[which];
  if (capacity < m || (m > 0 && !out)) return fail(DQ_ERR_SPACE, "dq_schema_selection: the buffer is too small");
  if (m > 0) DQ_HIP(hipMemcpy(out, s->d_sel[which].ptr, (size_t)m * 4, hipMemcpyDeviceToHost));
  return DQ_OK;
}

// Host build of the int and decimal cell tests (dq_schema.h, the source the evaluate kernel runs).
extern "C" dq_status dq_diag_schema_cell(int32_t kind, const uint8_t* text, int64_t n, int32_t precision, int32_t scale,
                                         int32_t* result, int64_t* value) {
  if ((!text && n > 0) || n < 0 || n > 0x7fffffff || !result || !value) return fail(DQ_ERR_INVALID, "bad argument");
  struct Text {
    const uint8_t* p;
    uint32_t operator[](int32_t i) const { return p[i]; }
  };
  *value = 0;
  if (kind == DQ_SCHEMA_INT) {
    int32_t v = 0;
    *result = schema::parse_int32(Text{text}, (int32_t)n, &v) ? schema::CELL_VALID : schema::CELL_INVALID;
    if (*result == schema::CELL_VALID) *value = v;
    return DQ_OK;
  }
  if (kind == DQ_SCHEMA_DECIMAL) {
    if (precision < 1 || precision > schema::kMaxDecimalPrecision || scale < 0 || scale > precision)
      return fail(DQ_ERR_INVALID, "dq_diag_schema_cell: needs 1 <= precision <= 18 and 0 <= scale <= precision");
    int64_t v = 0;
    *result = schema::parse_decimal(Text{text}, (int32_t)n, precision, scale, &v);
    if (*result == schema::CELL_VALID) *value = v;
    return DQ_OK;
  }
  return fail(DQ_ERR_INVALID, "dq_diag_schema_cell: kind is DQ_SCHEMA_INT or DQ_SCHEMA_DECIMAL");
}
