// dq_kll_api.inc -- the dq_kll_* family (include/deequ_amd.h): KLLSketch's runner.  Included by
// dq_api.cpp (fail, DQ_HIP, DevBuf, dq_ctx).  Per batch: one slab launch for every KLL column, the
// tree-merge rounds, then the batch's sketch per column comes to the host and is merged into the
// running one with the reference's sequential merge (dq_kll.cpp), in arrival order.

namespace dq {
hipError_t launch_kll_slabs(const kll::DevKllColumn* d_cols, int n_cols, int64_t n_rows, int64_t slab_rows,
                            int64_t n_slabs, uint32_t lds_bytes, kll::DevSketch* d_sketches, uint64_t* d_items,
                            hipStream_t stream);
hipError_t launch_kll_merge(const kll::DevKllColumn* d_cols, int n_cols, int64_t n_slabs, int64_t step, int pool_items,
                            uint32_t lds_bytes, kll::DevSketch* d_sketches, uint64_t* d_items, hipStream_t stream);
}  // namespace dq

struct KllColumnState {
  int32_t column = 0, sketch_size = 0;
  double shrinking_factor = 0;
  int32_t cap[kll::kMaxLevels];
  int64_t stride = 0;   // item keys per device sketch: the capacity of all kMaxLevels levels
  int32_t slab_pool = 0;
  std::unique_ptr<kll::Sketch> running;
  DevBuf values, validity;
};

struct dq_kll {
  int device = 0;
  std::vector<int32_t> types;
  std::vector<KllColumnState> cols;
  int64_t slab_rows = kll::kDefaultSlabRows;
  int32_t merge_pool = 0;
  DevBuf d_cols, d_sketches, d_items;
};

// The parameters the kernels can hold: every level's capacity known and positive, and two sketches'
// worth of all kMaxLevels levels resident in one workgroup's LDS (the tree merge).
static dq_status kll_check_params(int32_t k, double c, int32_t* cap, int64_t* sum) {
  kll::capacity_table(k, c, cap, sum);
  const int64_t bound = kll::kMaxPoolItems / 2;
  int64_t run = 0;
  for (int h = 0; h < kll::kMaxLevels && run <= bound; ++h) {  // (past the bound the Int capacities may have wrapped)
    if (cap[h] < 2)
      return fail(DQ_ERR_INVALID, "KLLSketch: sketchSize " + std::to_string(k) + " / shrinkingFactor " +
                                      std::to_string(c) + " give level " + std::to_string(h) + " the capacity " +
                                      std::to_string(cap[h]));
    run += cap[h];
  }
  if (run > bound) *sum = std::max(*sum, run);
  if (*sum > bound)
    return fail(DQ_ERR_UNSUPPORTED,
                "KLLSketch(sketchSize=" + std::to_string(k) + ", shrinkingFactor=" + std::to_string(c) + "): its " +
                    std::to_string(kll::kMaxLevels) + " levels hold " + std::to_string(*sum) +
                    " items; the GPU sketcher keeps two sketches in one workgroup's LDS and is bound to " +
                    std::to_string(bound) + " items per sketch (" + std::to_string(kll::kLdsBudgetBytes / 1024) +
                    " KiB of LDS)");
  return DQ_OK;
}

extern "C" dq_status dq_kll_supported(int32_t sketch_size, double shrinking_factor) {
  int32_t cap[kll::kMaxLevels];
  int64_t sum = 0;
  return kll_check_params(sketch_size, shrinking_factor, cap, &sum);
}

extern "C" dq_status dq_kll_create(dq_ctx* ctx, const dq_kll_column* columns, int n, const int32_t* column_types,
                                   int n_columns, int64_t slab_rows, dq_kll** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !columns || !column_types || n < 1 || n > 1024 || n_columns < 1)
    return fail(DQ_ERR_INVALID, "dq_kll_create: bad argument (1 to 1024 sketched columns)");
  if (slab_rows < 0 || slab_rows > ((int64_t)1 << 40)) return fail(DQ_ERR_INVALID, "dq_kll_create: slab_rows out of range");
  std::unique_ptr<dq_kll> s(new dq_kll());
  s->device = ctx->device;
  s->types.assign(column_types, column_types + n_columns);
  if (slab_rows > 0) s->slab_rows = slab_rows;
  s->cols.resize(n);
  int64_t widest = 0;
  for (int i = 0; i < n; ++i) {
    KllColumnState& c = s->cols[i];
    c.column = columns[i].column;
    c.sketch_size = columns[i].sketch_size;
    c.shrinking_factor = columns[i].shrinking_factor;
    if (c.column < 0 || c.column >= n_columns) return fail(DQ_ERR_INVALID, "dq_kll_create: column out of range");
    if (!is_numeric(column_types[c.column]))  // KLLRunner.scala:135-144: "Cannot handle <type>"
      return fail(DQ_ERR_INVALID, "dq_kll_create: column " + std::to_string(c.column) + " is not numeric");
    DQ_TRY(kll_check_params(c.sketch_size, c.shrinking_factor, c.cap, &c.stride));
    const int levels = kll::levels_bound(c.cap, s->slab_rows);
    int64_t pool = 1;
    for (int h = 0; h < levels; ++h) pool += c.cap[h];
    c.slab_pool = (int32_t)pool;
    widest = std::max(widest, c.stride);
  }
  s->merge_pool = (int32_t)std::min<int64_t>(kll::kMaxPoolItems, 2 * widest);
  *out = s.release();
  return DQ_OK;
}

extern "C" dq_status dq_kll_destroy(dq_kll* s) {
  delete s;
  return DQ_OK;
}

static std::unique_ptr<kll::Sketch> kll_from_device(const KllColumnState& c, const kll::DevSketch& h,
                                                    const std::vector<uint64_t>& keys) {
  std::unique_ptr<kll::Sketch> sk(new kll::Sketch(c.sketch_size, c.shrinking_factor));
  sk->levels.resize(h.n_levels);
  size_t at = 0;
  sk->actual = 0;
  sk->total = 0;
  for (int l = 0; l < h.n_levels; ++l) {
    kll::Compactor& lv = sk->levels[l];
    lv.num_compress = h.num_compress[l];
    lv.offset = h.offset[l];
    lv.buf.resize(h.len[l]);
    for (int i = 0; i < h.len[l]; ++i) lv.buf[i] = kll::value_of_key(keys[at + i]);
    at += h.len[l];
    sk->actual += h.len[l];
    sk->total += c.cap[l];
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  sk->min = h.has_nan ? nan : kll::value_of_key(h.min_key);  // math.min / math.max propagate NaN
  sk->max = h.has_nan ? nan : kll::value_of_key(h.max_key);
  return sk;
}

extern "C" dq_status dq_kll_consume(dq_kll* s, const dq_column* columns, int n_columns, int64_t n_rows) {
  if (!s || !columns || n_columns != (int)s->types.size() || n_rows < 0)
    return fail(DQ_ERR_INVALID, "dq_kll_consume: bad argument");
  DQ_HIP(hipSetDevice(s->device));
  const int n = (int)s->cols.size();
  const int64_t n_slabs = std::max<int64_t>(1, (n_rows + s->slab_rows - 1) / s->slab_rows);
  if (n_slabs > 0x7fffffff) return fail(DQ_ERR_INVALID, "dq_kll_consume: too many slabs in one batch");
  std::vector<kll::DevKllColumn> dc(n);
  int32_t slab_pool = 0;
  for (int i = 0; i < n; ++i) {
    KllColumnState& c = s->cols[i];
    const dq_column& col = columns[c.column];
    if (col.type != s->types[c.column]) return fail(DQ_ERR_INVALID, "dq_kll_consume: column type differs from the schema");
    if (col.length < n_rows || col.offset < 0) return fail(DQ_ERR_INVALID, "dq_kll_consume: column shorter than the batch");
    if (n_rows > 0 && !col.values) return fail(DQ_ERR_INVALID, "dq_kll_consume: values is NULL");
    const size_t w = (size_t)type_size(col.type);
    kll::DevKllColumn& d = dc[i];
    memset(&d, 0, sizeof(d));
    if (col.flags & DQ_COL_DEVICE) {
      d.values = static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w;
      d.validity = col.validity;
      d.bit_offset = col.offset;
    } else {
      DQ_TRY(c.values.ensure((size_t)n_rows * w));
      if (n_rows > 0)
        DQ_HIP(hipMemcpy(c.values.ptr, static_cast<const uint8_t*>(col.values) + (size_t)col.offset * w,
                         (size_t)n_rows * w, hipMemcpyHostToDevice));
      d.values = c.values.ptr;
      d.bit_offset = col.offset & 7;
      if (col.validity && n_rows > 0) {
        const size_t first = (size_t)(col.offset >> 3), bytes = (size_t)((d.bit_offset + n_rows + 7) >> 3);
        DQ_TRY(c.validity.ensure(bytes));
        DQ_HIP(hipMemcpy(c.validity.ptr, col.validity + first, bytes, hipMemcpyHostToDevice));
        d.validity = static_cast<const uint8_t*>(c.validity.ptr);
      }
    }
    d.type = col.type;
    d.pool_items = c.slab_pool;
    d.stride = c.stride;
    memcpy(d.cap, c.cap, sizeof(d.cap));
    slab_pool = std::max(slab_pool, c.slab_pool);
  }
  // one DevSketch array (column i's slabs from i * n_slabs) and one item array (column i's blocks of
  // its own stride from item_base)
  int64_t words = 0;
  for (int i = 0; i < n; ++i) {
    dc[i].sketch_base = (int64_t)i * n_slabs;
    dc[i].item_base = words;
    words += s->cols[i].stride * n_slabs;
  }
  const int64_t n_sketch = (int64_t)n * n_slabs;
  DQ_TRY(s->d_cols.ensure(sizeof(kll::DevKllColumn) * (size_t)n));
  DQ_TRY(s->d_sketches.ensure(sizeof(kll::DevSketch) * (size_t)n_sketch));
  DQ_TRY(s->d_items.ensure((size_t)words * 8));
  DQ_HIP(hipMemcpy(s->d_cols.ptr, dc.data(), sizeof(kll::DevKllColumn) * (size_t)n, hipMemcpyHostToDevice));
  const kll::DevKllColumn* d_cols = static_cast<const kll::DevKllColumn*>(s->d_cols.ptr);
  kll::DevSketch* d_sk = static_cast<kll::DevSketch*>(s->d_sketches.ptr);
  uint64_t* d_items = static_cast<uint64_t*>(s->d_items.ptr);
  DQ_HIP(launch_kll_slabs(d_cols, n, n_rows, s->slab_rows, n_slabs,
                          (uint32_t)(kll::kLdsReserveBytes + (size_t)slab_pool * 8), d_sk, d_items, nullptr));
  for (int64_t step = 1; step < n_slabs; step *= 2)
    DQ_HIP(launch_kll_merge(d_cols, n, n_slabs, step, s->merge_pool,
                            (uint32_t)(kll::kLdsReserveBytes + (size_t)s->merge_pool * 8), d_sk, d_items, nullptr));
  DQ_HIP(hipStreamSynchronize(nullptr));
  for (int i = 0; i < n; ++i) {
    KllColumnState& c = s->cols[i];
    kll::DevSketch h;
    DQ_HIP(hipMemcpy(&h, d_sk + dc[i].sketch_base, sizeof(h), hipMemcpyDeviceToHost));
    if (h.error || h.n_levels < 1 || h.n_levels > kll::kMaxLevels)
      return fail(DQ_ERR_UNSUPPORTED, h.error == 2 ? "KLLSketch: the sketch outgrew its " +
                                                          std::to_string(kll::kMaxLevels) + " levels"
                                                    : std::string("KLLSketch: the sketch's levels outgrew the LDS pool"));
    int64_t actual = 0;
    for (int l = 0; l < h.n_levels; ++l) {
      if (h.len[l] < 0) return fail(DQ_ERR_DEVICE, "KLLSketch: a corrupt device sketch");
      actual += h.len[l];
    }
    if (actual > c.stride) return fail(DQ_ERR_DEVICE, "KLLSketch: a corrupt device sketch");
    std::vector<uint64_t> keys((size_t)actual);
    if (actual > 0)
      DQ_HIP(hipMemcpy(keys.data(), d_items + dc[i].item_base, (size_t)actual * 8, hipMemcpyDeviceToHost));
    std::unique_ptr<kll::Sketch> batch = kll_from_device(c, h, keys);
    if (!c.running) c.running = std::move(batch);  // KLLState.sum in arrival order
    else c.running->merge_untyped(*batch);
  }
  return DQ_OK;
}

extern "C" dq_status dq_kll_finish(dq_kll* s, int64_t* sizes, int n) {
  if (!s || !sizes || n != (int)s->cols.size()) return fail(DQ_ERR_INVALID, "dq_kll_finish: bad argument");
  for (int i = 0; i < n; ++i) {
    KllColumnState& c = s->cols[i];
    if (!c.running) c.running.reset(new kll::Sketch(c.sketch_size, c.shrinking_factor));  // no batch: an empty sketch
    sizes[i] = c.running->export_words() * 8;
  }
  return DQ_OK;
}

extern "C" dq_status dq_kll_export(dq_kll* s, int i, void* out, int64_t capacity, int64_t* required) {
  if (!s || i < 0 || i >= (int)s->cols.size()) return fail(DQ_ERR_INVALID, "dq_kll_export: bad argument");
  KllColumnState& c = s->cols[i];
  if (!c.running) return fail(DQ_ERR_STATE, "dq_kll_export before dq_kll_finish");
  const int64_t need = c.running->export_words() * 8;
  if (required) *required = need;
  if (!out || capacity < need) return fail(DQ_ERR_SPACE, "dq_kll_export: the buffer is too small");
  c.running->export_to(out);
  return DQ_OK;
}

extern "C" dq_status dq_diag_kll_sketch(const double* values, const uint8_t* valid, int64_t n, int32_t sketch_size,
                                        double shrinking_factor, int64_t slab_rows, void* out, int64_t capacity,
                                        int64_t* required) {
  if (n < 0 || (n > 0 && !values) || slab_rows < 1) return fail(DQ_ERR_INVALID, "dq_diag_kll_sketch: bad argument");
  for (int h = 0; h < kll::kMaxLevels; ++h)
    if (kll::capacity(sketch_size, shrinking_factor, h) < 2)
      return fail(DQ_ERR_INVALID, "dq_diag_kll_sketch: a level without capacity");
  const kll::Sketch sk = kll::sketch_slabs(values, valid, n, sketch_size, shrinking_factor, slab_rows);
  const int64_t need = sk.export_words() * 8;
  if (required) *required = need;
  if (!out || capacity < need) return fail(DQ_ERR_SPACE, "dq_diag_kll_sketch: the buffer is too small");
  sk.export_to(out);
  return DQ_OK;
}
