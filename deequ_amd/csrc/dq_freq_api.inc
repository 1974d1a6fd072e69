// dq_freq_api.inc -- host side of the frequency group-by C-ABI (dq_freq_* in deequ_amd.h).
// Included at the end of dq_api.cpp (shares DevBuf, Stager, prepare_column, fail, DQ_HIP).
//
// A dq_freq is the device-resident FrequenciesAndNumRows (GroupingAnalyzers.scala:124-157).
// consume() = computeFrequencies over one batch (GroupingAnalyzers.scala:53-80), processed in
// sub-batches so the open-addressing table can be grown (rehashed) between them and never
// exceeds a 0.7 load factor; summary() derives every frequency metric from a count-of-counts
// histogram (integers, then a fixed summation order on the host: deterministic).

enum FreqCounter {
  FC_GROUPS = 0, FC_HEAP_USED, FC_OVERFLOW, FC_NEED, FC_NBIG, FC_EXPORT_N, FC_STAGED, FC_RETRY, FC_MAXLEN,
  FC_PART_OVF, FC_PART_FLAG, FC_IMP_RECS, FC_PACK_PROBE, FC_UUID_BAD, FC_UUID_GOOD, FC_PROBE_LONG, FC_SELECTED, FC_COUNT
};

// Distinct-key estimate of the staging sketch, used only to size the table.  This is the plain
// HLL estimator (2^-M in exact fp64 arithmetic, linear counting while registers are empty),
// NOT DeequHyperLogLogPlusPlusUtils.count: deequ's Java int shift `1 << M` wraps for M >= 31,
// so one high register collapses its estimate by orders of magnitude (a faithful quirk for
// ApproxCountDistinct, a sizing disaster here).
static double hll_estimate(const uint32_t* regs) {
  double z = 0.0;
  int zeros = 0;
  for (int i = 0; i < kHllM; ++i) {
    z += std::ldexp(1.0, -(int)regs[i]);
    zeros += regs[i] == 0u;
  }
  const double m = (double)kHllM;
  const double e = (0.7213 / (1.0 + 1.079 / m)) * m * m / z;
  if (zeros > 0 && e <= 2.5 * m) return m * std::log(m / (double)zeros);
  return e;
}

static int slice_bits_for(uint64_t capacity) {
  int b = 0;
  while ((kFreqSliceSlots << b) < capacity) ++b;
  return b;
}

struct dq_freq : Stager {
  dq_ctx* ctx = nullptr;
  FreqKeySpec ks{};
  int flags = 0;
  bool has_utf8 = false;
  std::vector<bool> col_used;
  uint64_t capacity = 0;  // slots (power of two)
  DevBuf d_slots, d_ctr, d_heap, d_cols, d_hist, d_big, d_out, d_in, d_part;
  // sorted-bucket path: staged records, their sketch, and the bucket split's work buffers
  // (d_keys_a: per-slice cursors, d_keys_b: level-1 counts / starts / cursors, d_sort_tmp: scan sums)
  DevBuf d_stage, d_sorted, d_keys_a, d_keys_b, d_sort_tmp, d_off, d_pieces, d_sketch;
  // partition path: level-1 regions, slice regions, their fill counters, the overflow list
  DevBuf d_part1, d_part2, d_pfill, d_pfill2, d_povf, d_smax, d_sketch_save;
  // set by a partition-path aggregation into an empty table: d_hist / d_big / FC_NBIG hold the
  // table's count-of-counts (no hist scan needed), d_smax each slice's largest count
  bool dev_hist_valid = false, smax_valid = false;
  // Compacted (round 6): the packed aggregation into an empty table wrote only the occupied slots
  // into d_slots (FreqCompact: d_cmeta holds base / num / occupancy bits / cursor per slice).
  // summary() and top() read that form; everything that probes or scans the slot image calls
  // expand() first (materialize() does), which rebuilds the exact image.  DQ_FREQ_COMPACT=0: off.
  bool compact = false;
  bool compact_enabled = true;
  DevBuf d_cmeta;
  uint64_t staged = 0;
  bool sorted_path = true;                   // DQ_FREQ_PATH=atomic disables it (tests)
  bool part_path = true;                     // DQ_FREQ_PART=0 disables the partition passes (tests)
  uint64_t part_min = (uint64_t)1 << 22;     // staged records below this take the sort (DQ_FREQ_PART_MIN)
  double part_load = 0.5;                    // sizing load of a partition-path table (DQ_FREQ_PART_LOAD)
  uint64_t part_slots = 0;                   // DQ_FREQ_PART_SLOTS test knob: that table size instead
  // Region staging (partition path for large stagings): the stage kernel writes every record
  // straight into its level-1 region (kRegionBits top hash bits) of d_part1, cap1 records each,
  // fills in d_pfill[0 .. 2^kRegionBits), a copy for rolling a batch back after them; records
  // beyond a region's room go to the overflow list d_povf (FC_PART_OVF).
  static constexpr int kRegionBits = 9;
  bool region_staged = false;                // the staged records are in d_part1's regions
  // A single utf8 key column stages digit keys as packed 8-byte records (dq_keypack.h) in the
  // regions; a batch whose other keys overflow the overflow list turns this off for the table.
  bool pack_default = true;                  // DQ_FREQ_PACK=0 disables (tests, A/B)
  DevBuf d_rows;                             // the row-order records of the batch being staged
  bool pack_keys = true;
  bool pack_probed = false;                  // the first packed staging sampled its keys (pack probe)
  bool len_probed = false;                   // a multi-column table's first staging sampled its key lengths
  bool region_packed = false;                // the regions' records are packed words
  // Long (> 15 B) and multi-column keys (round 6): the table stages HashRec records {table hash,
  // reference to the key's bytes, copied into the key heap by the stage} once a batch held such a
  // key; region_hashed: the staged regions hold them.  DQ_FREQ_HASHED=0: the per-row insert path.
  bool hash_keys = false, hashed_enabled = true, region_hashed = false;
  uint64_t diag_hashed_runs = 0, diag_hashed_inserts = 0;
  // Keys whose bytes fit two words (round 6): a single utf8 key column whose sampled keys are all
  // canonical UUIDs (dq_uuidpack.h) stages UuidRec records {the key's 128 bits}; one whose sampled
  // keys are all 16 bytes long, or two 8-byte fixed-width key columns, stage Raw16Rec records {the
  // key's 16 bytes} -- instead of hashed ones.  wide_keys: the form this table stages (kRecUuid /
  // kRecRaw16, 0 = hashed records); region_wide: the form the staged regions hold (region_hashed
  // is set too).  A batch holding a key the form cannot hold is rolled back and the table stages
  // hashed records from then on.  DQ_FREQ_UUID=0 disables both forms (tests, A/B).
  bool uuid_enabled = true, uuid_probed = false;
  int wide_keys = 0, region_wide = 0;
  uint64_t diag_uuid_runs = 0, diag_raw16_runs = 0;
  static constexpr uint64_t kUuidHeapBytes = 40;  // a group's text in the heap (36 bytes, 8-aligned)
  uint64_t region_rows = 0;                  // rows the regions were sized for (0 = none)
  uint64_t cap1 = 0, ovf_cap = 0;
  uint64_t reserve_rows = 0;                 // dq_freq_reserve hint
  bool debug = false;                        // DQ_FREQ_DEBUG=1: sizing/retry trace on stderr
  bool test_no_publish = false;              // dq_diag_freq_test_flags(kFreqTestNoPublish): a broken publish (tests)
  // which paths the groupings took (dq_diag_freq_paths; tests assert on them)
  uint64_t diag_part_runs = 0, diag_sort_records = 0, diag_packed_runs = 0;
  uint64_t diag_import_coarse = 0, diag_import_skipped = 0;  // wire runs cut at coarser slices / inserted one by one
  int diag_part_bits = 0;
  // batches rolled back out of the regions / regions aggregated because a batch of another record format arrived
  uint64_t diag_rollbacks = 0, diag_materialized_for_format = 0;
  // derived views, valid until the table changes (consume / import / merge / reset)
  bool hist_valid = false;
  std::vector<unsigned long long> hist_cache, big_cache;  // count-of-counts (freq_hist)
  int top_n = -1;                                          // dq_freq_top's last result
  std::vector<std::pair<unsigned long long, std::string>> top_cache;
  // dq_freq_export_flat's device result, kept from the sizing call to the filling call
  DevBuf d_flat_aux, d_flat, d_flat_bytes;
  DevBuf d_dist;  // dq_freq_linf_distance's eight result words
  DevBuf d_probe;  // dq_freq_probe_rows' "count == 1" words of the batch
  bool flat_valid = false;
  uint64_t flat_n = 0, flat_bytes = 0;
  // Cross-table checks: d_row_of_slot[s] = the row (dq_freq_index_rows) that holds slot s's key, -1
  // where none was indexed; one int64 per slot, alive while index_valid.  A slot keeps its place
  // only until the table changes, so whatever changes it or moves its slots drops the index.
  // d_match: the index's absent counter, the match's four counters, then its compare columns.
  static constexpr size_t kMatchHeadBytes = 64;
  DevBuf d_row_of_slot, d_match;
  bool index_valid = false;
  void drop_index() {
    index_valid = false;
    d_row_of_slot.release();
  }
  void invalidate() {
    drop_index();
    flat_valid = false;
    hist_valid = false;
    dev_hist_valid = false;
    smax_valid = false;
    top_n = -1;
    top_cache.clear();
  }
  uint64_t stage_budget = (uint64_t)1 << 30;  // records staged before an early aggregation
  int64_t num_rows = 0;
  int64_t sub_rows = (int64_t)1 << 26;  // rows per insert launch (multiple of 8)
  int64_t few_groups = 0;               // dq_freq_expect_groups hint (<= kFreqFewGroups), 0 = none
  bool few_only = false;                // DQ_FREQ_FEW_ONLY: the few-groups kernel or DQ_ERR_SPACE
  bool few_failed = false;              // a DQ_FREQ_FEW_ONLY batch did not fit: every consume fails
  std::vector<DevColumn> h_cols;
  // The table's `where` (dq_freq_set_filter): one validated program, uploaded once.  Every batch
  // evaluates it into d_fwords {TRUE words, NOT NULL words} (LIKE / RLIKE: match masks first, into
  // d_fmatch_words) and folds the TRUE words into the first key column's validity (d_fvalid), so
  // every path below sees a filtered-out row as a NULL key.  The selected rows are counted on the
  // device (FC_SELECTED, a running total); read_counters settles it into num_rows, in the read
  // every path makes after staging: rows_pending says that a batch is not settled yet.
  bool filtered = false, filter_cast = false, rows_pending = false;
  uint32_t filter_lds = 0;
  int filter_matches = 0;
  unsigned long long rows_settled = 0;  // of FC_SELECTED, already in num_rows
  std::vector<DevColumn> filter_cols;
  DevBuf d_fprog, d_finsns, d_fpool, d_fmatch, d_fdfas, d_fcols, d_fwords, d_fmatch_words, d_fvalid;

  ~dq_freq() {
    if (stream) StreamPool::get().release(ctx ? ctx->device : 0, stream);
    stream = nullptr;
    PinnedPool::get().release(h_ctr);
  }

  unsigned long long* ctr() { return static_cast<unsigned long long*>(d_ctr.ptr); }

  FreqTable view() {
    FreqTable T;
    T.slots = static_cast<FreqSlot*>(d_slots.ptr);
    T.mask = capacity - 1;
    T.bucket_bits = slice_bits_for(capacity);
    T.test_flags = test_no_publish ? kFreqTestNoPublish : 0;
    T.n_groups = ctr() + FC_GROUPS;
    T.heap = static_cast<uint8_t*>(d_heap.ptr);
    T.heap_used = ctr() + FC_HEAP_USED;
    T.heap_cap = d_heap.cap;
    T.overflow = reinterpret_cast<unsigned int*>(ctr() + FC_OVERFLOW);
    return T;
  }

  // The counters come back through a pinned buffer: a copy to pageable memory is staged by the
  // runtime and costs tens of microseconds more, and a table reads its counters several times
  // per batch.
  unsigned long long* h_ctr = nullptr;
  dq_status read_counters(unsigned long long* h) {
    if (!h_ctr) DQ_HIP(PinnedPool::get().alloc(FC_COUNT * sizeof(unsigned long long), reinterpret_cast<void**>(&h_ctr)));
    DQ_HIP(hipMemcpyAsync(h_ctr, d_ctr.ptr, FC_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    std::memcpy(h, h_ctr, FC_COUNT * sizeof(unsigned long long));
    if (filtered) {  // the selected rows of the batches consumed since the last read
      num_rows += (int64_t)(h[FC_SELECTED] - rows_settled);
      rows_settled = h[FC_SELECTED];
      rows_pending = false;
    }
    return DQ_OK;
  }
  // num_rows is current: a filtered table's last batches may be counted on the device only.
  dq_status settle_rows() {
    if (!rows_pending) return DQ_OK;
    unsigned long long h[FC_COUNT];
    return read_counters(h);
  }
  dq_status apply_filter(int n_columns, int64_t n_rows);

  // Grow to keep (groups + incoming) below a 0.6 load factor (per-slice loads scatter around
  // the mean: at 0.6 a 2048-slot slice is 5 sigma away from full).
  dq_status ensure_capacity(uint64_t groups, uint64_t incoming, bool clear = true) {
    const uint64_t target = groups + incoming;
    if (target * 10 <= capacity * 6) return DQ_OK;
    uint64_t cap = capacity;
    while (target * 10 > cap * 5) cap <<= 1;  // land at <= 0.5 after growing
    return grow_to(cap, clear || groups > 0);
  }
  FreqCompact cmeta() {
    const uint64_t n_slices = capacity >> kFreqSliceLog;
    uint8_t* p = static_cast<uint8_t*>(d_cmeta.ptr);
    FreqCompact c;
    c.slots = static_cast<FreqSlot*>(d_slots.ptr);
    c.base = reinterpret_cast<unsigned long long*>(p);
    c.cursor = c.base + n_slices;
    c.num = reinterpret_cast<uint32_t*>(c.cursor + 1);
    c.bits = reinterpret_cast<uint8_t*>(c.num + n_slices);
    return c;
  }
  static size_t cmeta_bytes(uint64_t n_slices) { return n_slices * (8 + 4 + 256) + 8; }

  // The slot image of a compacted table, rebuilt (into a fresh buffer: the compact groups are
  // read from d_slots while it is written).
  dq_status expand() {
    if (!compact) return DQ_OK;
    DevBuf fresh;
    DQ_TRY(fresh.ensure(capacity * sizeof(FreqSlot)));
    FreqTable T = view();
    T.slots = static_cast<FreqSlot*>(fresh.ptr);
    DQ_HIP(launch_freq_expand(T, cmeta(), stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_slots.swap(fresh);
    compact = false;
    table_cleared = true;
    drop_index();
    return DQ_OK;
  }

  dq_status clear_table() {
    if (compact) return DQ_OK;  // (d_slots holds the compacted groups: expand() writes the image whole)
    if (!table_cleared) DQ_HIP(hipMemsetAsync(d_slots.ptr, 0, capacity * sizeof(FreqSlot), stream));
    table_cleared = true;
    return DQ_OK;
  }

  // clear = false (an empty table about to be written whole by the partition path): the new
  // slots are left uninitialised and table_cleared says so.
  bool table_cleared = true;
  dq_status grow_to(uint64_t cap, bool clear = true) {
    DQ_TRY(expand());
    DevBuf fresh;
    DQ_TRY(fresh.ensure(cap * sizeof(FreqSlot)));
    smax_valid = false;  // the slice layout changes
    if (clear) DQ_HIP(hipMemsetAsync(fresh.ptr, 0, cap * sizeof(FreqSlot), stream));
    table_cleared = clear;
    FreqTable T = view();
    T.slots = static_cast<FreqSlot*>(fresh.ptr);
    T.mask = cap - 1;
    T.bucket_bits = slice_bits_for(cap);
    if (capacity) DQ_HIP(launch_freq_rehash(static_cast<const FreqSlot*>(d_slots.ptr), capacity, T, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_slots.swap(fresh);
    capacity = cap;
    drop_index();
    return DQ_OK;
  }

  dq_status ensure_heap(uint64_t used, uint64_t need) {
    if (used + need <= d_heap.cap) return DQ_OK;
    size_t cap = std::max<size_t>(d_heap.cap * 2, used + need + (1u << 20));
    DevBuf fresh;
    DQ_TRY(fresh.ensure(cap));
    if (used) DQ_HIP(hipMemcpyAsync(fresh.ptr, d_heap.ptr, used, hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_heap.swap(fresh);
    return DQ_OK;
  }

  // The staged records aggregated and the table's slot image valid: what every operation that
  // probes or scans slots needs.
  dq_status materialize() {
    DQ_TRY(aggregate());
    return expand();
  }
  // materialize() for an operation that is about to change the table.  The derived views are
  // dropped after it, not before: its own aggregation, when it runs on the partition path into an
  // empty table, marks the count-of-counts and the slice maxima valid, and they would then
  // describe the table as it was before the operation's rows.
  dq_status materialize_for_write() {
    DQ_TRY(materialize());
    invalidate();
    return DQ_OK;
  }

  // Aggregate the staged records into the table: group them by slice (bucket split), one work item per slice's bucket
  // (a bucket of more than kAggPiece records is split into atomically merged pieces).  The table may
  // be left compacted (summary / top read that form; materialize() expands it).
  dq_status aggregate() {
    if (staged == 0) return DQ_OK;
    DQ_TRY(expand());  // (the records go into the groups already there)
    if (region_staged && region_hashed) return aggregate_hashed();
    std::vector<uint32_t> regs(kHllM);
    DQ_HIP(hipMemcpyAsync(regs.data(), d_sketch.ptr, kHllM * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    const double est = hll_estimate(regs.data());
    const uint64_t expect = std::min<uint64_t>(staged, (uint64_t)(est * 1.25) + 4096);
    int table_empty = h[FC_GROUPS] == 0 ? 1 : 0;
    uint64_t n = staged;
    const bool partition = region_staged || (part_path && n >= part_min);
    if (partition && table_empty) {
      // an empty table that the partition path writes whole: not cleared first, and sized so
      // that 1.15x the sketch's estimate is at most a part_load (0.5) load.  Fuller tables write
      // fewer bytes but probe longer in LDS: 0.92 measured 12 ms slower per C4 step than 0.37.
      // The hard limit is a slice's 2048 LDS slots: at a true load of 0.9 the fullest of 2^17
      // slices is still ~4 sigma short of it, and a slice that does fill up goes through the sort
      // path's retry (correct, slower).
      const uint64_t target = std::min<uint64_t>(staged, (uint64_t)(est * 1.15) + 4096);
      uint64_t cap = capacity;
      while ((double)target > part_load * (double)cap) cap <<= 1;
      if (part_slots) cap = std::max<uint64_t>(capacity, part_slots);  // (tests: slices that overflow LDS)
      if (cap > capacity) DQ_TRY(grow_to(cap, false));
    } else {
      DQ_TRY(ensure_capacity(h[FC_GROUPS], expect));
    }
    FreqRec* src_recs = static_cast<FreqRec*>(d_stage.ptr);
    if (partition) {
      bool used = false;
      DQ_TRY(partition_and_aggregate(n, est, table_empty, h[FC_PART_OVF], used, src_recs, n));
      if (used) table_empty = 0;
    }
    if (n > 0) DQ_TRY(expand());  // (retried records are aggregated into the slot image)
    DQ_TRY(clear_table());
    if (n > 0) {  // the bucket-split rounds change counts the fused histogram / slice maxima do not see
      dev_hist_valid = false;
      smax_valid = false;
    }
    FreqRec* cur = src_recs;  // the records still to aggregate (n of them)
    for (int round = 0; n > 0; ++round) {
      if (round == 8) return fail(DQ_ERR_DEVICE, "frequency table: groups could not be placed (internal)");
      diag_sort_records += n;
      const uint64_t n_buckets = capacity >> kFreqSliceLog;
      int bits = 0;
      while ((1ull << bits) < n_buckets) ++bits;
      if (bits < 1 || bits > 2 * kPartMaxBits) return fail(DQ_ERR_DEVICE, "frequency table: slice count out of range (internal)");
      // group the records by slice (the bucket split): cur -> [tmp ->] grouped; the buffer left
      // free takes the rows of slices that fill up in LDS (retry)
      const int b2 = bits > kPartMaxBits ? bits - kPartMaxBits : 0;
      const uint64_t r1 = 1ull << (bits - b2);
      DQ_TRY(d_off.ensure((n_buckets + 1) * sizeof(unsigned long long)));
      DQ_TRY(d_pieces.ensure((n_buckets + 1) * sizeof(uint32_t)));
      DQ_TRY(d_keys_a.ensure(n_buckets * sizeof(unsigned long long)));                 // slice cursors
      DQ_TRY(d_keys_b.ensure(3 * (r1 + 1) * sizeof(unsigned long long)));             // level 1: counts / starts / cursors
      DQ_TRY(d_sort_tmp.ensure(((n_buckets + 1) / 4096 + 2) * sizeof(unsigned long long)));  // scan chunk sums
      FreqRec* other;  // a second buffer of >= n records that cur does not live in
      if (cur == static_cast<FreqRec*>(d_sorted.ptr)) {
        DQ_TRY(d_stage.ensure(n * sizeof(FreqRec)));
        other = static_cast<FreqRec*>(d_stage.ptr);
      } else {
        DQ_TRY(d_sorted.ensure(n * sizeof(FreqRec)));
        other = static_cast<FreqRec*>(d_sorted.ptr);
      }
      unsigned long long* cnt = static_cast<unsigned long long*>(d_off.ptr);  // per-slice counts, then starts
      unsigned long long* cursor = static_cast<unsigned long long*>(d_keys_a.ptr);
      unsigned long long* c1 = static_cast<unsigned long long*>(d_keys_b.ptr);
      unsigned long long* off1 = c1 + (r1 + 1);
      unsigned long long* cur1 = off1 + (r1 + 1);
      unsigned long long* sums = static_cast<unsigned long long*>(d_sort_tmp.ptr);
      uint32_t* pieces = static_cast<uint32_t*>(d_pieces.ptr);
      FreqRec* grouped;
      FreqRec* retry;
      DQ_HIP(hipMemsetAsync(cnt, 0, (n_buckets + 1) * sizeof(unsigned long long), stream));
      if (b2 == 0) {  // one level: the level-1 bins are the slices
        DQ_HIP(launch_freq_split(cur, n, nullptr, 0, 0, bits, 0, cnt, nullptr, nullptr, nullptr, stream));
      } else {  // level 1 by the top bits into exact regions (other), then the slices' counts inside them
        DQ_HIP(hipMemsetAsync(c1, 0, 3 * (r1 + 1) * sizeof(unsigned long long), stream));
        DQ_HIP(launch_freq_split(cur, n, nullptr, 0, 0, bits, b2, c1, nullptr, nullptr, nullptr, stream));
        std::vector<unsigned long long> hc(r1), ho(r1 + 1);
        DQ_HIP(hipMemcpyAsync(hc.data(), c1, r1 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        DQ_HIP(hipStreamSynchronize(stream));
        uint64_t run = 0, biggest = 0;
        for (uint64_t r = 0; r < r1; ++r) {
          ho[r] = run;
          run += hc[r];
          biggest = std::max<uint64_t>(biggest, hc[r]);
        }
        ho[r1] = run;
        DQ_HIP(hipMemcpyAsync(off1, ho.data(), (r1 + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
        DQ_HIP(launch_freq_split(cur, n, nullptr, 0, 0, bits, b2, nullptr, other, off1, cur1, stream));
        DQ_HIP(launch_freq_split(other, 0, off1, r1, biggest, bits, b2, cnt, nullptr, nullptr, nullptr, stream));
        DQ_HIP(hipStreamSynchronize(stream));  // (the host vectors above die here)
      }
      // per-slice counts -> work items and exact slice starts
      DQ_HIP(launch_freq_pieces(cnt, n_buckets, pieces, stream));
      DQ_HIP(scan_exclusive_u32(pieces, n_buckets + 1, reinterpret_cast<uint32_t*>(sums), stream));
      DQ_HIP(scan_exclusive_u64(cnt, n_buckets + 1, sums, stream));
      DQ_HIP(hipMemsetAsync(cursor, 0, n_buckets * sizeof(unsigned long long), stream));
      if (b2 == 0) {
        DQ_HIP(launch_freq_split(cur, n, nullptr, 0, 0, bits, 0, nullptr, other, cnt, cursor, stream));
        grouped = other;
        retry = cur;
      } else {
        std::vector<unsigned long long> ho(r1 + 1);
        DQ_HIP(hipMemcpyAsync(ho.data(), off1, (r1 + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        DQ_HIP(hipStreamSynchronize(stream));
        uint64_t biggest = 0;
        for (uint64_t r = 0; r < r1; ++r) biggest = std::max<uint64_t>(biggest, ho[r + 1] - ho[r]);
        DQ_HIP(launch_freq_split(other, 0, off1, r1, biggest, bits, b2, nullptr, cur, cnt, cursor, stream));
        grouped = cur;
        retry = other;
      }
      if (debug) {  // host-side checks of the grouping and the work-item numbering
        std::vector<unsigned long long> ho(n_buckets + 1);
        std::vector<uint32_t> hp(n_buckets + 1);
        DQ_HIP(hipMemcpyAsync(ho.data(), cnt, ho.size() * 8, hipMemcpyDeviceToHost, stream));
        DQ_HIP(hipMemcpyAsync(hp.data(), pieces, hp.size() * 4, hipMemcpyDeviceToHost, stream));
        DQ_HIP(hipStreamSynchronize(stream));
        uint64_t bad_off = 0, bad_scan = 0;
        for (uint64_t b = 0; b < n_buckets; ++b) {
          bad_off += ho[b] > ho[b + 1];
          bad_scan += hp[b + 1] - hp[b] != (uint32_t)((ho[b + 1] - ho[b] + kFreqAggPiece - 1) / kFreqAggPiece);
        }
        std::fprintf(stderr, "[dq_freq] split check: n %llu bits %d b2 %d bad_off %llu bad_scan %llu grouped %llu items %u\n",
                     (unsigned long long)n, bits, b2, (unsigned long long)bad_off, (unsigned long long)bad_scan,
                     ho[n_buckets], hp[n_buckets]);
      }
      DQ_HIP(hipMemsetAsync(ctr() + FC_RETRY, 0, sizeof(unsigned long long), stream));
      const uint64_t max_items = n_buckets + n / kFreqAggPiece + 1;
      DQ_HIP(launch_freq_agg(view(), grouped, reinterpret_cast<const uint64_t*>(cnt), pieces, n_buckets, max_items,
                             table_empty, retry, ctr() + FC_RETRY, ctr() + FC_GROUPS, stream));
      DQ_TRY(read_counters(h));
      if (h[FC_OVERFLOW] & kFreqWaitTimeout) return check_overflow();
      if (debug)
        std::fprintf(stderr, "[dq_freq] materialize round %d: records %llu, sketch est %.0f, capacity %llu, "
                     "groups %llu, retry %llu\n", round, (unsigned long long)n, est, (unsigned long long)capacity,
                     h[FC_GROUPS], h[FC_RETRY]);
      n = h[FC_RETRY];
      cur = retry;
      table_empty = 0;
      if (n) {  // some slices were full: make room for every returned row as a new group
        const uint64_t before = capacity;
        DQ_TRY(ensure_capacity(h[FC_GROUPS], n));
        if (capacity == before) DQ_TRY(grow_to(capacity * 2));
      }
    }
    staged = 0;
    DQ_HIP(hipMemsetAsync(d_sketch.ptr, 0, kHllM * sizeof(uint32_t), stream));
    DQ_HIP(hipMemsetAsync(ctr() + FC_STAGED, 0, sizeof(unsigned long long), stream));
    DQ_HIP(hipStreamSynchronize(stream));
    // staging and sort buffers are as large as the staged rows: back to the device block pool
    d_stage.release();
    d_sorted.release();
    d_keys_a.release();
    d_keys_b.release();
    d_sort_tmp.release();
    d_part1.release();
    d_part2.release();
    d_povf.release();
    d_rows.release();
    region_staged = false;
    region_rows = 0;
    return DQ_OK;
  }

  // The region-staged records laid out contiguously in d_stage (+ the n_ovf overflowed ones),
  // for the paths that need them so: few slices (bits < kRegionBits), very many (P2 beyond
  // kPartMaxBinBits bits), or an overflow list that filled up in P2.  Afterwards the staging is
  // an ordinary contiguous one.
  dq_status compact_regions(uint64_t n_ovf, uint64_t& n_out) {
    const uint64_t r1 = 1ull << kRegionBits;
    std::vector<unsigned long long> fill(r1), prefix(r1);
    DQ_HIP(hipMemcpyAsync(fill.data(), d_pfill.ptr, r1 * 8, hipMemcpyDeviceToHost, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    uint64_t total = 0;
    for (uint64_t r = 0; r < r1; ++r) {
      prefix[r] = total;
      total += std::min<uint64_t>(fill[r], cap1);
    }
    n_out = total + n_ovf;
    DQ_TRY(d_stage.ensure(std::max<uint64_t>(1, n_out) * sizeof(FreqRec)));
    unsigned long long* d_prefix = static_cast<unsigned long long*>(d_pfill.ptr) + 2 * r1;
    DQ_HIP(hipMemcpyAsync(d_prefix, prefix.data(), r1 * 8, hipMemcpyHostToDevice, stream));
    DQ_HIP(launch_freq_compact(d_part1.ptr, region_packed, static_cast<const unsigned long long*>(d_pfill.ptr), cap1, r1,
                               d_prefix, static_cast<FreqRec*>(d_stage.ptr), stream));
    if (n_ovf)
      DQ_HIP(hipMemcpyAsync(static_cast<FreqRec*>(d_stage.ptr) + total, d_povf.ptr, n_ovf * sizeof(FreqRec),
                            hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_part1.release();
    region_staged = false;
    region_rows = 0;
    return DQ_OK;
  }

  // Regions for a staging of up to `rows` rows (region staging); fills and overflow zeroed.
  dq_status alloc_regions(uint64_t rows) {
    const uint64_t r1 = 1ull << kRegionBits;
    cap1 = region_cap(rows, r1, 8.0);
    ovf_cap = rows / 16 + 65536;
    DQ_TRY(d_part1.ensure(r1 * cap1 * sizeof(FreqRec)));
    DQ_TRY(d_pfill.ensure(3 * r1 * sizeof(unsigned long long)));
    DQ_TRY(d_povf.ensure(ovf_cap * sizeof(FreqRec)));
    DQ_HIP(hipMemsetAsync(d_pfill.ptr, 0, 3 * r1 * sizeof(unsigned long long), stream));
    DQ_HIP(hipMemsetAsync(ctr() + FC_PART_OVF, 0, 2 * sizeof(unsigned long long), stream));  // + FC_PART_FLAG
    region_rows = rows;
    return DQ_OK;
  }

  // Begin staging a batch of n_rows rows into the regions.  compatible: the regions staged so
  // far hold the record format this batch stages; a contiguous staging, or regions of another
  // format, are aggregated first.  The regions are (re)allocated when the batch does not fit.
  // Then the fills, the sizing sketch and the overflow count are saved on the device (one small
  // kernel: no host round trip before the launch; a rolled-back batch's hashes must not inflate
  // the table's size) and the batch's longest-key counter is cleared.
  dq_status begin_region_stage(int64_t n_rows, bool compatible) {
    if (staged > 0 && !(region_staged && compatible)) {
      if (region_staged) ++diag_materialized_for_format;  // (else a contiguous staging: no format to change)
      DQ_TRY(materialize());
    }
    if (region_rows == 0 || staged + (uint64_t)n_rows > region_rows) {
      if (staged > 0) DQ_TRY(materialize());
      DQ_TRY(alloc_regions(std::max<uint64_t>((uint64_t)n_rows, reserve_rows)));
    }
    const uint64_t r1 = 1ull << kRegionBits;
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    DQ_TRY(d_sketch_save.ensure(kHllM * sizeof(uint32_t) + sizeof(unsigned long long)));
    uint8_t* sk_save = static_cast<uint8_t*>(d_sketch_save.ptr);
    DQ_HIP(launch_freq_stage_save(fill1, fill1 + r1, (uint32_t)r1, static_cast<const uint32_t*>(d_sketch.ptr),
                                  reinterpret_cast<uint32_t*>(sk_save), ctr() + FC_PART_OVF,
                                  reinterpret_cast<unsigned long long*>(sk_save + kHllM * sizeof(uint32_t)),
                                  ctr() + FC_MAXLEN, stream));
    return DQ_OK;
  }

  // Roll a batch back: the fills, the sketch and the overflow count as begin_region_stage saved
  // them, the overflow flag cleared, the staged count as it was, and the heap cursor back at
  // *heap_used (the hashed stage; nullptr: the heap was not written).
  dq_status rollback_region_stage(const unsigned long long* heap_used) {
    ++diag_rollbacks;
    const uint64_t r1 = 1ull << kRegionBits;
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    const uint8_t* sk_save = static_cast<const uint8_t*>(d_sketch_save.ptr);
    DQ_HIP(hipMemcpyAsync(fill1, fill1 + r1, r1 * 8, hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipMemcpyAsync(d_sketch.ptr, sk_save, kHllM * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipMemcpyAsync(ctr() + FC_PART_OVF, sk_save + kHllM * sizeof(uint32_t), sizeof(unsigned long long),
                          hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipMemsetAsync(ctr() + FC_PART_FLAG, 0, sizeof(unsigned long long), stream));
    DQ_HIP(hipMemcpyAsync(ctr() + FC_STAGED, &staged, sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    if (heap_used)
      DQ_HIP(hipMemcpyAsync(ctr() + FC_HEAP_USED, heap_used, sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    return DQ_OK;
  }

  // Stage a batch into the regions (dq_freq_stage_packed_rows_kernel for packed records,
  // dq_freq_stage_part_kernel for 16-byte ones).  staged_ok = false: the batch
  // holds a key this path cannot stage (longer than 15 bytes) or overflowed the overflow list;
  // it has been rolled back and the caller groups it on the general path.
  dq_status stage_regions(int64_t n_rows, bool& staged_ok) {
    staged_ok = false;
    if (hash_keys) return stage_hashed(n_rows, staged_ok);
    const bool one_string = ks.n_keys == 1 && col_types[ks.key_cols[0]] == DQ_T_UTF8;
    if (ks.n_keys > 1 && !len_probed && hashed_enabled && staged == 0) {
      // a multi-column key: if sampled rows already encode to more than 15 bytes the batch would
      // be staged as 16-B records and rolled back -- stage hashed records from the start
      len_probed = true;
      DQ_HIP(hipMemsetAsync(ctr() + FC_PROBE_LONG, 0, sizeof(unsigned long long), stream));
      DQ_HIP(launch_freq_len_probe(ks, static_cast<const DevColumn*>(d_cols.ptr), n_rows, ctr() + FC_PROBE_LONG, stream));
      unsigned long long hp[FC_COUNT];
      DQ_TRY(read_counters(hp));
      if (hp[FC_PROBE_LONG] > 0) {
        if (debug) std::fprintf(stderr, "[dq_freq] length probe: %llu sampled keys over 15 bytes: hashed records\n",
                                hp[FC_PROBE_LONG]);
        hash_keys = true;
        pack_keys = false;
        return stage_hashed(n_rows, staged_ok);
      }
    }
    if (pack_keys && one_string && !pack_probed) {
      // the table's first packed staging: sample the batch's keys first -- a column whose keys
      // mostly are not digit strings would fill the packed stage's overflow list (rows / 16) and
      // be staged twice, so it stages 16-B records from the start
      pack_probed = true;
      DQ_HIP(hipMemsetAsync(ctr() + FC_PACK_PROBE, 0, sizeof(unsigned long long), stream));
      DQ_HIP(hipMemsetAsync(ctr() + FC_PROBE_LONG, 0, sizeof(unsigned long long), stream));
      DQ_HIP(launch_freq_pack_probe(ks, static_cast<const DevColumn*>(d_cols.ptr), n_rows, ctr() + FC_PACK_PROBE, stream,
                                    ctr() + FC_PROBE_LONG));
      unsigned long long hp[FC_COUNT];
      DQ_TRY(read_counters(hp));
      if (hp[FC_PROBE_LONG] > 0 && hashed_enabled && staged == 0) {
        // sampled keys longer than a 16-byte record holds: the batch would be staged, then rolled
        // back -- the table stages hashed (or UUID) records from the start
        if (debug) std::fprintf(stderr, "[dq_freq] pack probe: %llu sampled keys over 15 bytes: hashed records\n",
                                hp[FC_PROBE_LONG]);
        hash_keys = true;
        pack_keys = false;
        return stage_hashed(n_rows, staged_ok);
      }
      // pack unless the estimated keys that do not pack (with a 25 % margin) would fill the packed
      // stage's overflow list (rows / 16 + 65536 records, alloc_regions)
      const uint64_t samples = std::min<uint64_t>((uint64_t)n_rows, 16384u);
      const double est = (double)hp[FC_PACK_PROBE] / (double)samples * (double)n_rows;
      if (est * 1.25 > (double)n_rows / 16.0 + 65536.0) {
        pack_keys = false;
        if (debug) std::fprintf(stderr, "[dq_freq] pack probe: %llu of %llu sampled keys do not pack: 16-B records\n",
                                (unsigned long long)hp[FC_PACK_PROBE], (unsigned long long)samples);
      }
    }
    const bool packed = pack_keys && one_string;
    DQ_TRY(begin_region_stage(n_rows, region_packed == packed && !region_hashed));
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    region_packed = packed;  // (nothing staged, or staged in this format)
    region_hashed = false;
    // row-order staging + the level-1 split (dq_freq_stage_packed_rows_kernel) for packed 8-B
    // records; 16-B records take the fused kernel: split, they move twice the extra bytes (alnum C4,
    // alternated on one box: 46.7 ms split against 40.3 fused, profiles/r05_c4_alnum_stage_ab.txt)
    const DevColumn* dcols = static_cast<const DevColumn*>(d_cols.ptr);
    FreqRec* ovf = static_cast<FreqRec*>(d_povf.ptr);
    unsigned int* flag = reinterpret_cast<unsigned int*>(ctr() + FC_PART_FLAG);
    uint32_t* sketch = static_cast<uint32_t*>(d_sketch.ptr);
    if (packed) {
      DQ_TRY(d_rows.ensure((size_t)n_rows * sizeof(uint64_t)));
      DQ_HIP(launch_freq_stage_packed_rows(ks, dcols, n_rows, kRegionBits, static_cast<uint64_t*>(d_rows.ptr),
                                           static_cast<uint64_t*>(d_part1.ptr), cap1, fill1, ovf, ctr() + FC_PART_OVF,
                                           ovf_cap, flag, sketch, ctr() + FC_MAXLEN, ctr() + FC_STAGED, stream));
    } else {
      DQ_HIP(launch_freq_stage_part(ks, one_string, dcols, n_rows, kRegionBits, static_cast<FreqRec*>(d_part1.ptr), cap1,
                                    fill1, ovf, ctr() + FC_PART_OVF, ovf_cap, flag, sketch, ctr() + FC_MAXLEN,
                                    ctr() + FC_STAGED, stream));
    }
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    if (h[FC_MAXLEN] <= 15 && h[FC_PART_FLAG] == 0) {
      staged = h[FC_STAGED];
      region_staged = staged > 0;
      staged_ok = true;
      return DQ_OK;
    }
    DQ_TRY(rollback_region_stage(nullptr));
    if (packed && h[FC_MAXLEN] <= 15) {
      // packed: the overflow list filled up, mostly with keys that are not digit strings -- this
      // table's keys are staged as 16-B records from now on (the packed regions are aggregated first)
      if (debug) std::fprintf(stderr, "[dq_freq] packed staging rolled back: 16-B records from now on\n");
      pack_keys = false;
      return stage_regions(n_rows, staged_ok);
    }
    if (hashed_enabled && h[FC_MAXLEN] > 15 && h[FC_MAXLEN] <= (unsigned long long)kMaxLocalKey) {
      // a key longer than a 16-B record holds: this table stages hashed records from now on
      if (debug) std::fprintf(stderr, "[dq_freq] key of %llu+ bytes: hashed records from now on\n", h[FC_MAXLEN]);
      hash_keys = true;
      pack_keys = false;
      return stage_hashed(n_rows, staged_ok);
    }
    return DQ_OK;
  }

  // Stage a batch of canonical UUID keys as UuidRec records straight into the level-1 regions
  // (dq_freq_stage_uuid_kernel).  A batch holding a non-NULL key that is not a canonical UUID, or
  // whose overflow list filled up, is rolled back; the table stages hashed records from then on
  // (the UUID regions already staged are aggregated first).
  dq_status stage_wide(int64_t n_rows, bool& staged_ok) {
    staged_ok = false;
    DQ_TRY(begin_region_stage(n_rows, region_wide == wide_keys));
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    DQ_HIP(hipMemsetAsync(ctr() + FC_UUID_BAD, 0, sizeof(unsigned long long), stream));
    region_packed = false;
    region_hashed = true;
    region_wide = wide_keys;
    if (wide_keys == kRecUuid)
      DQ_HIP(launch_freq_stage_uuid(ks, static_cast<const DevColumn*>(d_cols.ptr), n_rows, kRegionBits, d_part1.ptr, cap1,
                                    fill1, static_cast<FreqRec*>(d_povf.ptr), ctr() + FC_PART_OVF, ovf_cap,
                                    reinterpret_cast<unsigned int*>(ctr() + FC_PART_FLAG),
                                    static_cast<uint32_t*>(d_sketch.ptr), ctr() + FC_UUID_BAD, ctr() + FC_STAGED, stream));
    else
      DQ_HIP(launch_freq_stage_raw16(ks, ks.n_keys == 1, static_cast<const DevColumn*>(d_cols.ptr), n_rows, kRegionBits,
                                     d_part1.ptr, cap1, fill1, static_cast<FreqRec*>(d_povf.ptr), ctr() + FC_PART_OVF,
                                     ovf_cap, reinterpret_cast<unsigned int*>(ctr() + FC_PART_FLAG),
                                     static_cast<uint32_t*>(d_sketch.ptr), ctr() + FC_UUID_BAD, ctr() + FC_STAGED, stream));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    if (h[FC_UUID_BAD] == 0 && h[FC_PART_FLAG] == 0) {
      staged = h[FC_STAGED];
      region_staged = staged > 0;
      staged_ok = true;
      return DQ_OK;
    }
    DQ_TRY(rollback_region_stage(nullptr));
    if (debug)
      std::fprintf(stderr, "[dq_freq] %s staging rolled back (%llu other keys, flag %llu): hashed records from now on\n",
                   wide_keys == kRecUuid ? "uuid" : "16-byte", h[FC_UUID_BAD], h[FC_PART_FLAG]);
    wide_keys = 0;
    if (staged == 0) {
      region_wide = 0;
      region_hashed = false;
    }
    return stage_hashed(n_rows, staged_ok);
  }

  // Stage a batch of long / multi-column keys as hashed records: key bytes into the heap (exact
  // size reserved first), records in row order, then the level-1 split into the regions.  A
  // multi-column key over kMaxLocalKey bytes, or a hot key that overflows the overflow list, rolls
  // the batch back (the heap cursor included) and the caller groups it on the general path.
  dq_status stage_hashed(int64_t n_rows, bool& staged_ok) {
    staged_ok = false;
    const bool one_key_string = ks.n_keys == 1 && col_types[ks.key_cols[0]] == DQ_T_UTF8;
    auto fixed8 = [&](int c) { const int t = col_types[ks.key_cols[c]]; return t == DQ_T_INT64 || t == DQ_T_FLOAT64; };
    const bool two_fixed8 = ks.n_keys == 2 && fixed8(0) && fixed8(1);
    if (uuid_enabled && !ks.null_as_key && (one_key_string || two_fixed8)) {
      if (!uuid_probed) {  // the table's first long-key staging: do its keys fit two words?
        uuid_probed = true;
        if (two_fixed8) {
          wide_keys = kRecRaw16;  // (the encoding is always the two values' 16 bytes)
        } else {
          DQ_HIP(hipMemsetAsync(ctr() + FC_UUID_BAD, 0, 2 * sizeof(unsigned long long), stream));
          DQ_HIP(hipMemsetAsync(ctr() + FC_PROBE_LONG, 0, sizeof(unsigned long long), stream));
          DQ_HIP(launch_freq_uuid_probe(ks, static_cast<const DevColumn*>(d_cols.ptr), n_rows, ctr() + FC_UUID_BAD, stream));
          DQ_HIP(launch_freq_len16_probe(ks, static_cast<const DevColumn*>(d_cols.ptr), n_rows, ctr() + FC_PROBE_LONG,
                                         stream));
          unsigned long long hp[FC_COUNT];
          DQ_TRY(read_counters(hp));
          const uint64_t sampled = hp[FC_UUID_BAD] + hp[FC_UUID_GOOD];
          wide_keys = hp[FC_UUID_BAD] == 0 && hp[FC_UUID_GOOD] > 0 ? kRecUuid
                      : (sampled > 0 && hp[FC_PROBE_LONG] == 0) ? kRecRaw16 : 0;
          if (debug)
            std::fprintf(stderr, "[dq_freq] long-key probe: %llu canonical UUIDs, %llu other, %llu not 16 bytes\n",
                         hp[FC_UUID_GOOD], hp[FC_UUID_BAD], hp[FC_PROBE_LONG]);
        }
      }
      if (wide_keys) return stage_wide(n_rows, staged_ok);
    }
    DQ_TRY(begin_region_stage(n_rows, region_hashed && !region_wide));
    const DevColumn* dcols = static_cast<const DevColumn*>(d_cols.ptr);
    unsigned long long h0[FC_COUNT];
    DQ_TRY(read_counters(h0));
    // An upper bound of the batch's heap bytes from the key columns' sizes (string bytes from the
    // first and last offsets; each key padded by < 8 bytes; a NULL's "NullValue" 16): when the
    // heap already has that room (every batch of a reserved job but the last few) the exact
    // count -- a pass over every key's length -- is skipped.
    uint64_t bound = 7ull * (uint64_t)n_rows + (ks.null_as_key ? 16ull * (uint64_t)n_rows : 0ull);
    for (int i = 0; i < ks.n_keys; ++i) {
      const DevColumn& c = h_cols[ks.key_cols[i]];
      if (c.type == DQ_T_UTF8) {
        int32_t ends[2];
        DQ_HIP(hipMemcpy(&ends[0], c.offsets, sizeof(int32_t), hipMemcpyDeviceToHost));
        DQ_HIP(hipMemcpy(&ends[1], c.offsets + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost));
        bound += (uint64_t)(uint32_t)(ends[1] - ends[0]) + (ks.n_keys > 1 ? 4ull * (uint64_t)n_rows : 0ull);
      } else {
        bound += (uint64_t)(type_size(c.type) ? type_size(c.type) : 1) * (uint64_t)n_rows;  // (bool: 1 byte)
      }
    }
    if (d_heap.cap < h0[FC_HEAP_USED] + bound) {
      DQ_HIP(hipMemsetAsync(ctr() + FC_NEED, 0, sizeof(unsigned long long), stream));
      DQ_HIP(launch_freq_key_bytes(ks, dcols, n_rows, ctr() + FC_NEED, stream));
      DQ_TRY(read_counters(h0));
      uint64_t need = h0[FC_NEED];
      if (reserve_rows > (uint64_t)n_rows && d_heap.cap < h0[FC_HEAP_USED] + need)  // room for the reserved rows at once
        need = (uint64_t)((double)need * ((double)reserve_rows / (double)n_rows) * 1.02);
      DQ_TRY(ensure_heap(h0[FC_HEAP_USED], need));
    }
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    region_packed = false;
    region_hashed = true;
    DQ_TRY(d_rows.ensure((size_t)n_rows * sizeof(HashRec)));
    HashRec* rows = static_cast<HashRec*>(d_rows.ptr);
    const bool one_string = ks.n_keys == 1 && col_types[ks.key_cols[0]] == DQ_T_UTF8;
    DQ_HIP(launch_freq_stage_hashed(ks, one_string, dcols, n_rows, rows, view(), static_cast<uint32_t*>(d_sketch.ptr),
                                    ctr() + FC_MAXLEN, nullptr, nullptr, stream));
    DQ_HIP(launch_freq_part(rows, (uint64_t)n_rows, nullptr, 0, 0, kRegionBits, kRegionBits, d_part1.ptr, cap1, fill1,
                            static_cast<FreqRec*>(d_povf.ptr), ctr() + FC_PART_OVF, ovf_cap,
                            reinterpret_cast<unsigned int*>(ctr() + FC_PART_FLAG), kRecHashed, stream, ctr() + FC_STAGED));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    if (h[FC_MAXLEN] <= (unsigned long long)kMaxLocalKey && h[FC_PART_FLAG] == 0 && !(h[FC_OVERFLOW] & 2u)) {
      staged = h[FC_STAGED];
      region_staged = staged > 0;
      staged_ok = true;
      return DQ_OK;
    }
    DQ_TRY(rollback_region_stage(&h0[FC_HEAP_USED]));  // (the heap cursor too)
    if (debug)
      std::fprintf(stderr, "[dq_freq] hashed staging rolled back (max len %llu, flag %llu)\n", h[FC_MAXLEN],
                   h[FC_PART_FLAG]);
    if (staged == 0) region_hashed = false;
    return DQ_OK;
  }

  // Aggregate hashed regions: a fresh table is sized like the partition path's and takes the LDS
  // aggregation (dq_freq_agg_hashed_kernel); records it hands back (a slice full, two keys of one
  // hash, a region overflow), and every record when the table already has groups, are inserted
  // globally from their heap bytes (exact key compares).
  dq_status aggregate_hashed() {
    const int wide_in = region_wide;  // (the regions hold UuidRec / Raw16Rec records)
    std::vector<uint32_t> regs(kHllM);
    DQ_HIP(hipMemcpyAsync(regs.data(), d_sketch.ptr, kHllM * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    const double est = hll_estimate(regs.data());
    const int table_empty = h[FC_GROUPS] == 0 ? 1 : 0;
    if (table_empty) {
      const uint64_t target = std::min<uint64_t>(staged, (uint64_t)(est * 1.15) + 4096);
      uint64_t cap = capacity;
      while ((double)target > part_load * (double)cap) cap <<= 1;
      if (part_slots) cap = std::max<uint64_t>(capacity, part_slots);
      if (cap > capacity) DQ_TRY(grow_to(cap, false));
    } else {
      DQ_TRY(ensure_capacity(h[FC_GROUPS], std::min<uint64_t>(staged, (uint64_t)(est * 1.25) + 4096)));
    }
    if (wide_in == kRecUuid && table_empty) {
      // the groups' text, written by the aggregation: at most one group per staged record and per
      // slot, expected the sketch's estimate (a slice that finds no room is handed back)
      const uint64_t groups = std::min<uint64_t>(std::min<uint64_t>(staged, capacity), (uint64_t)(est * 1.3) + 65536);
      DQ_TRY(ensure_heap(h[FC_HEAP_USED], groups * kUuidHeapBytes));
    }
    bool used = false;
    FreqRec* rest = nullptr;
    uint64_t n_rest = 0;
    DQ_TRY(partition_and_aggregate(staged, est, table_empty, h[FC_PART_OVF], used, rest, n_rest));
    if (wide_in) {
      DQ_TRY(read_counters(h));
      if (h[FC_HEAP_USED] > d_heap.cap) {  // slices that found no heap room left a reservation past the end
        const unsigned long long cap = d_heap.cap;
        DQ_HIP(hipMemcpyAsync(ctr() + FC_HEAP_USED, &cap, sizeof(cap), hipMemcpyHostToDevice, stream));
        DQ_HIP(hipStreamSynchronize(stream));
        h[FC_HEAP_USED] = cap;
      }
      if (n_rest > 0) {  // the records left over are key bits: the key bytes into the heap, hashed records
        DQ_TRY(ensure_heap(h[FC_HEAP_USED], n_rest * (wide_in == kRecUuid ? kUuidHeapBytes : 16ull)));
        DQ_HIP(launch_freq_uuid_to_hashed(view(), rest, n_rest, stream, wide_in));
      }
    }
    if (!used) {  // nothing aggregated: every record (laid out contiguously) is inserted globally
      DQ_TRY(clear_table());
      dev_hist_valid = false;
      smax_valid = false;
    }
    if (n_rest > 0) {
      DQ_TRY(expand());
      DQ_TRY(clear_table());
      dev_hist_valid = false;
      smax_valid = false;
      unsigned long long hg[FC_COUNT];
      DQ_TRY(read_counters(hg));
      DQ_TRY(ensure_capacity(hg[FC_GROUPS], n_rest));  // (every record left over may be a new group)
      DQ_HIP(launch_freq_insert_hashed(view(), rest, n_rest, stream));
      diag_hashed_inserts += n_rest;
    }
    DQ_TRY(check_overflow());
    staged = 0;
    DQ_HIP(hipMemsetAsync(d_sketch.ptr, 0, kHllM * sizeof(uint32_t), stream));
    DQ_HIP(hipMemsetAsync(ctr() + FC_STAGED, 0, sizeof(unsigned long long), stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_stage.release();
    d_part1.release();
    d_part2.release();
    d_povf.release();
    d_rows.release();
    region_staged = false;
    region_hashed = false;
    region_wide = 0;
    region_rows = 0;
    return DQ_OK;
  }

  // Region capacity: the expected share of n over `regions` plus a 6-sigma margin.  Records of
  // one key land together, so the spread is that of a sum of per-key counts: variance ~ mean x
  // (rows per distinct key).
  static uint64_t region_cap(uint64_t n, uint64_t regions, double dup) {
    const double mean = (double)n / (double)regions;
    const double c = mean + 6.0 * std::sqrt(mean * std::max(1.0, dup)) + 64.0;
    return ((uint64_t)c + 63u) & ~(uint64_t)63u;
  }

  // The partition path over the n staged records: P1 (stage -> level-1 regions), P2 (-> slice
  // regions), one owner aggregation per slice region.  used = false (nothing changed) when it does
  // not apply or its overflow list filled up (the caller sorts the staged records instead).
  // Otherwise `rest` / `n_rest` are the records still to aggregate: those of slices that filled up
  // in LDS and those beyond a region's capacity (normally none).
  // n_ovf_staged: records the region staging put on the overflow list (region_staged only).
  dq_status partition_and_aggregate(uint64_t n, double est, int table_empty, uint64_t n_ovf_staged, bool& used,
                                    FreqRec*& rest, uint64_t& n_rest) {
    used = false;
    rest = static_cast<FreqRec*>(d_stage.ptr);  // (when not used: what the sort path takes)
    n_rest = n;
    const bool hashed_in = region_staged && region_hashed;  // (hashed records never reach the sort path)
    const uint64_t n_slices = capacity >> kFreqSliceLog;
    int bits = 0;
    while ((1ull << bits) < n_slices) ++bits;
    if (region_staged && (bits < kRegionBits || bits - kRegionBits > kPartMaxBits || bits > 22 ||
                          (region_hashed && !table_empty))) {
      // the regions do not match this table's slices (or hold hashed records for a table that
      // already has groups: the hashed aggregation writes fresh tables only): lay the staging out
      // contiguously again (hashed records: the caller inserts them globally)
      DQ_TRY(compact_regions(n_ovf_staged, n));
      staged = n;
      rest = static_cast<FreqRec*>(d_stage.ptr);
      n_rest = n;
      if (hashed_in) return DQ_OK;  // (the caller inserts them globally)
    }
    if (bits < 1 || bits > 22) return DQ_OK;
    const bool from_regions = region_staged;
    const bool pk = from_regions && region_packed;  // the regions hold packed digit records
    const bool hk = from_regions && region_hashed;  // ... hashed records of long keys
    const int rk = hk && region_wide ? region_wide : hk ? kRecHashed : pk ? kRecPacked : kRecFree;  // (wide: UUID / 16-byte records)
    const size_t rec_bytes = pk ? sizeof(uint64_t) : sizeof(FreqRec);
    const int b1 = from_regions ? kRegionBits : (bits <= 9 ? bits : std::max(9, bits - kPartMaxBits));
    const int b2 = bits - b1;
    const uint64_t r1 = 1ull << b1, r2 = b2 ? (1ull << bits) : 0;
    const double dup = (double)n / std::max(1.0, est);
    const uint64_t c1 = from_regions ? cap1 : region_cap(n, r1, dup), cap2 = b2 ? region_cap(n, r2, dup) : 0;
    const uint64_t ocap = from_regions ? ovf_cap : n / 16 + 65536;
    if (!from_regions) {
      DQ_TRY(d_part1.ensure(r1 * c1 * sizeof(FreqRec)));
      DQ_TRY(d_povf.ensure(ocap * sizeof(FreqRec)));
      DQ_TRY(d_pfill.ensure(r1 * sizeof(unsigned long long)));
    }
    if (b2) DQ_TRY(d_part2.ensure(r2 * cap2 * rec_bytes));
    DQ_TRY(d_pfill2.ensure(std::max<uint64_t>(1, r2) * sizeof(unsigned long long)));
    unsigned long long* fill1 = static_cast<unsigned long long*>(d_pfill.ptr);
    unsigned long long* fill2 = static_cast<unsigned long long*>(d_pfill2.ptr);
    void* p1 = d_part1.ptr;  // (at least r1 * c1 16-B records: the retry list when P2 runs)
    void* p2 = d_part2.ptr;
    FreqRec* ovf = static_cast<FreqRec*>(d_povf.ptr);
    unsigned int* flag = reinterpret_cast<unsigned int*>(ctr() + FC_PART_FLAG);
    if (r2) DQ_HIP(hipMemsetAsync(fill2, 0, r2 * sizeof(unsigned long long), stream));
    if (!from_regions) {
      DQ_HIP(hipMemsetAsync(d_pfill.ptr, 0, r1 * sizeof(unsigned long long), stream));
      DQ_HIP(hipMemsetAsync(ctr() + FC_PART_OVF, 0, 2 * sizeof(unsigned long long), stream));  // + FC_PART_FLAG
      DQ_HIP(launch_freq_part(static_cast<const FreqRec*>(d_stage.ptr), n, nullptr, 0, 0, b1, b1, p1, c1, fill1, ovf,
                              ctr() + FC_PART_OVF, ocap, flag, false, stream));
    }
    if (b2)
      DQ_HIP(launch_freq_part(p1, 0, fill1, c1, r1, bits, b2, p2, cap2, fill2, ovf, ctr() + FC_PART_OVF, ocap, flag,
                              rk, stream));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    if (debug)
      std::fprintf(stderr, "[dq_freq] partition%s: n %llu bits %d b1 %d b2 %d cap1 %llu cap2 %llu overflow %llu flag %llu\n",
                   from_regions ? " (region staged)" : "", (unsigned long long)n, bits, b1, b2,
                   (unsigned long long)c1, (unsigned long long)cap2, h[FC_PART_OVF], h[FC_PART_FLAG]);
    if (h[FC_PART_FLAG]) {  // skewed beyond the overflow list: sort the staged records instead
      if (from_regions) {
        uint64_t m = 0;
        DQ_TRY(compact_regions(n_ovf_staged, m));
        staged = m;
        rest = static_cast<FreqRec*>(d_stage.ptr);
        n_rest = m;
      }
      d_part1.release();
      d_part2.release();
      d_povf.release();
      return DQ_OK;
    }
    // slice regions -> table; rows of a slice that fills up in LDS go to the retry buffer (the
    // level-1 regions, free once P2 has run; the staging buffer when there is no P2).  Into an
    // empty table the aggregation also counts the count-of-counts and each slice's maximum.
    const void* regions = b2 ? p2 : p1;
    if (!b2) DQ_TRY(d_stage.ensure(std::max<uint64_t>(1, n) * sizeof(FreqRec)));
    FreqRec* retry = static_cast<FreqRec*>(b2 ? p1 : d_stage.ptr);
    unsigned long long *hist = nullptr, *big = nullptr;
    uint32_t* smax = nullptr;
    const uint64_t big_cap = n / kFreqHist + 1;
    if (table_empty) {
      DQ_TRY(d_big.ensure(big_cap * sizeof(unsigned long long)));
      DQ_TRY(d_smax.ensure(n_slices * sizeof(uint32_t)));
      hist = static_cast<unsigned long long*>(d_hist.ptr);
      big = static_cast<unsigned long long*>(d_big.ptr);
      smax = static_cast<uint32_t*>(d_smax.ptr);
      DQ_HIP(hipMemsetAsync(hist, 0, kFreqHist * sizeof(unsigned long long), stream));
      DQ_HIP(hipMemsetAsync(ctr() + FC_NBIG, 0, sizeof(unsigned long long), stream));
    }
    if (!table_empty) {  // (the fused counts are those of an aggregation into an empty table)
      dev_hist_valid = false;
      smax_valid = false;
    }
    DQ_HIP(hipMemsetAsync(ctr() + FC_RETRY, 0, sizeof(unsigned long long), stream));
    // packed records into a fresh table: only the occupied slots are written (the table is
    // compacted; expand() rebuilds the slot image for the operations that probe)
    const bool to_compact = compact_enabled && table_empty && !table_cleared;
    FreqCompact cmp{};
    if (to_compact) {
      DQ_TRY(d_cmeta.ensure(cmeta_bytes(n_slices)));
      cmp = cmeta();
      DQ_HIP(hipMemsetAsync(cmp.cursor, 0, sizeof(unsigned long long), stream));
    }
    DQ_HIP(launch_freq_agg_region(view(), regions, rk, b2 ? fill2 : fill1, b2 ? cap2 : c1, n_slices, table_empty, retry,
                                  ctr() + FC_RETRY, ctr() + FC_GROUPS, hist, big, ctr() + FC_NBIG, big_cap, smax,
                                  (table_empty && !table_cleared) ? 1 : 0, stream, to_compact ? &cmp : nullptr));
    if (to_compact) compact = true;   // (expand() writes every slot of the image it rebuilds)
    if (table_empty) table_cleared = true;  // every slot written (or, compacted, to be written whole)
    DQ_TRY(read_counters(h));
    const uint64_t k = h[FC_RETRY], m = h[FC_PART_OVF];
    if (table_empty && k + m == 0) {
      dev_hist_valid = true;
      smax_valid = true;
    }
    if (m) DQ_HIP(hipMemcpyAsync(retry + k, ovf, m * sizeof(FreqRec), hipMemcpyDeviceToDevice, stream));
    if (debug)
      std::fprintf(stderr, "[dq_freq] partition: groups %llu, slice retry %llu, region overflow %llu\n",
                   h[FC_GROUPS], (unsigned long long)k, (unsigned long long)m);
    DQ_HIP(hipStreamSynchronize(stream));
    d_part2.release();
    d_povf.release();
    d_rows.release();
    region_staged = false;
    region_rows = 0;
    used = true;
    ++diag_part_runs;
    if (pk) ++diag_packed_runs;
    if (hk) ++diag_hashed_runs;
    if (rk == kRecUuid) ++diag_uuid_runs;
    if (rk == kRecRaw16) ++diag_raw16_runs;
    diag_part_bits = bits;
    rest = retry;
    n_rest = k + m;
    return DQ_OK;
  }

  // Room for `rows` more staged records (and their sort keys), keeping what is staged; growth
  // is at least `factor` x the current capacity.
  dq_status reserve_stage(uint64_t rows, uint64_t factor) {
    const uint64_t need = staged + rows;
    if (need * sizeof(FreqRec) <= d_stage.cap) return DQ_OK;
    const uint64_t recs = std::max<uint64_t>(need, factor * (d_stage.cap / sizeof(FreqRec)));
    DevBuf fresh;
    DQ_TRY(fresh.ensure(recs * sizeof(FreqRec)));
    if (staged)
      DQ_HIP(hipMemcpyAsync(fresh.ptr, d_stage.ptr, staged * sizeof(FreqRec), hipMemcpyDeviceToDevice, stream));
    DQ_HIP(hipStreamSynchronize(stream));
    d_stage.swap(fresh);
    return DQ_OK;
  }

  // ---- merges: the key-hash exchange's receiver and dq_freq_merge (dq_freq.hip "Key-hash
  // exchange and table merges").  runs: the record streams; incoming_exact >= 0: the number of
  // distinct incoming keys is known (a source table's groups), else it is sketched; heap_bytes:
  // the long-key bytes the runs may add to the key heap.
  DevBuf d_imp_runs, d_imp_bounds, d_imp_ovf;
  DevBuf d_small;                   // few-groups staging lists (dq_freq_small_kernel)
  bool small_path = true;           // DQ_FREQ_SMALL=0 disables it (tests, A/B)
  uint64_t diag_small_runs = 0;
  dq_status import_runs(std::vector<ImportRun>& runs, int64_t incoming_exact, uint64_t heap_bytes) {
    DQ_TRY(materialize_for_write());
    uint64_t max_n = 0;
    bool general = false;  // a run that may hold keys the LDS image cannot (kind 1 / 2)
    for (const ImportRun& r : runs) {
      max_n = std::max<uint64_t>(max_n, r.n);
      general = general || r.kind != 0;
    }
    if (runs.empty() || max_n == 0) return DQ_OK;
    const int n_runs = (int)runs.size();
    if (n_runs > 65535) return fail(DQ_ERR_INVALID, "too many parts to import");
    DQ_TRY(d_imp_runs.ensure(runs.size() * sizeof(ImportRun)));
    ImportRun* d_runs = static_cast<ImportRun*>(d_imp_runs.ptr);
    DQ_HIP(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(ImportRun), hipMemcpyHostToDevice, stream));
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    uint64_t incoming = incoming_exact >= 0 ? (uint64_t)incoming_exact : 0;
    if (incoming_exact < 0) {  // (the staging sketch is zero after materialize)
      DQ_HIP(launch_import_sketch(d_runs, n_runs, max_n, static_cast<uint32_t*>(d_sketch.ptr), stream));
      std::vector<uint32_t> regs(kHllM);
      DQ_HIP(hipMemcpyAsync(regs.data(), d_sketch.ptr, kHllM * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      DQ_HIP(hipMemsetAsync(d_sketch.ptr, 0, kHllM * sizeof(uint32_t), stream));
      DQ_HIP(hipStreamSynchronize(stream));
      incoming = (uint64_t)(hll_estimate(regs.data()) * 1.15) + 4096;
    }
    DQ_TRY(ensure_heap(h[FC_HEAP_USED], heap_bytes));
    int table_empty = h[FC_GROUPS] == 0 ? 1 : 0;
    if (table_empty) {  // sized like the partition path's tables, written whole (no clearing)
      uint64_t cap = capacity;
      while ((double)incoming > part_load * (double)cap) cap <<= 1;
      if (part_slots) cap = std::max<uint64_t>(capacity, part_slots);  // (tests: slices that overflow LDS)
      if (cap > capacity) DQ_TRY(grow_to(cap, false));
    } else {
      DQ_TRY(ensure_capacity(h[FC_GROUPS], incoming));
    }
    const int rb = slice_bits_for(capacity);
    const uint64_t n_slices = capacity >> kFreqSliceLog;
    // slice boundaries of the wire runs; a run found out of order is imported group by group
    bool any_wire = false;
    for (const ImportRun& r : runs) any_wire = any_wire || r.kind != 2;
    uint32_t* d_start = nullptr;
    uint32_t* d_end = nullptr;
    const size_t bound_words = any_wire ? (size_t)n_runs * n_slices : 0;
    DQ_TRY(d_imp_bounds.ensure(std::max<size_t>(1, 2 * bound_words) * sizeof(uint32_t) + 8 * (size_t)n_runs));
    unsigned int* d_unsorted = reinterpret_cast<unsigned int*>(static_cast<uint32_t*>(d_imp_bounds.ptr) + 2 * bound_words);
    unsigned int* d_drop = d_unsorted + n_runs;
    if (any_wire) {
      d_start = static_cast<uint32_t*>(d_imp_bounds.ptr);
      d_end = d_start + bound_words;
      for (ImportRun& r : runs) r.bits = rb;  // cut at the receiver's slices first
      DQ_HIP(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(ImportRun), hipMemcpyHostToDevice, stream));
      DQ_HIP(hipMemsetAsync(d_imp_bounds.ptr, 0, 2 * bound_words * sizeof(uint32_t) + 8 * (size_t)n_runs, stream));
      DQ_HIP(launch_import_bounds(d_runs, n_runs, max_n, rb, n_slices, d_start, d_end, d_unsorted, d_drop, 0, stream));
      std::vector<unsigned int> uns(2 * (size_t)n_runs);
      DQ_HIP(hipMemcpyAsync(uns.data(), d_unsorted, 8 * (size_t)n_runs, hipMemcpyDeviceToHost, stream));
      DQ_HIP(hipStreamSynchronize(stream));
      // A run in order only by coarser slices than ours (a sender with fewer slice bits, or one
      // that sorted by chunks of slices) is cut at those coarser slices instead -- each of our
      // slices then reads its enclosing range and filters -- when that costs at most 2^3 reads
      // of its records; a run that is not in order at all is inserted group by group.
      constexpr unsigned int kMaxDrop = 3;
      bool changed = false, coarse = false;
      for (int i = 0; i < n_runs; ++i) {
        if (!uns[i]) continue;
        changed = true;
        const unsigned int drop = uns[n_runs + i];
        if (drop <= kMaxDrop && (int)drop <= rb) {
          runs[i].bits = rb - (int)drop;
          coarse = true;
          ++diag_import_coarse;
          const size_t row = (size_t)i * n_slices;
          DQ_HIP(hipMemsetAsync(d_start + row, 0, n_slices * sizeof(uint32_t), stream));
          DQ_HIP(hipMemsetAsync(d_end + row, 0, n_slices * sizeof(uint32_t), stream));
        } else {
          runs[i].skip = 1;
          ++diag_import_skipped;
        }
      }
      if (changed)
        DQ_HIP(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(ImportRun), hipMemcpyHostToDevice, stream));
      if (coarse)
        DQ_HIP(launch_import_bounds(d_runs, n_runs, max_n, rb, n_slices, d_start, d_end, d_unsorted, d_drop, 1, stream));
      if (debug && changed)
        std::fprintf(stderr, "[dq_freq] import: runs out of slice order: cut at coarser slices or inserted group by group\n");
    }
    bool packed = true, any_skip = false;
    for (const ImportRun& r : runs) {
      if (!r.skip && r.kind != 0) packed = false;
      any_skip = any_skip || r.skip;
    }
    // the slice-owner merge (into an empty table it also counts the count-of-counts and each
    // slice's maximum, as the partition path's aggregation does)
    unsigned long long *hist = nullptr, *big = nullptr;
    uint32_t* smax = nullptr;
    uint64_t total_n = 0;
    for (const ImportRun& r : runs) total_n += r.n;
    const uint64_t big_cap = total_n / kFreqHist + 1;
    if (table_empty) {
      DQ_TRY(d_big.ensure(big_cap * sizeof(unsigned long long)));
      DQ_TRY(d_smax.ensure(n_slices * sizeof(uint32_t)));
      hist = static_cast<unsigned long long*>(d_hist.ptr);
      big = static_cast<unsigned long long*>(d_big.ptr);
      smax = static_cast<uint32_t*>(d_smax.ptr);
      DQ_HIP(hipMemsetAsync(hist, 0, kFreqHist * sizeof(unsigned long long), stream));
      DQ_HIP(hipMemsetAsync(ctr() + FC_NBIG, 0, sizeof(unsigned long long), stream));
    }
    DQ_TRY(d_imp_ovf.ensure(n_slices * sizeof(uint32_t)));
    DQ_HIP(hipMemsetAsync(ctr() + FC_RETRY, 0, sizeof(unsigned long long), stream));
    DQ_HIP(hipMemsetAsync(ctr() + FC_IMP_RECS, 0, sizeof(unsigned long long), stream));
    bool flat = packed && n_runs <= kImportFlatRuns;  // every run a packed wire run, none skipped
    for (const ImportRun& r : runs) flat = flat && r.kind == 0 && !r.skip;
    DQ_HIP(launch_import_merge(view(), packed, flat, d_runs, n_runs, d_start, d_end, table_empty, hist, big, ctr() + FC_NBIG,
                               big_cap, smax, (table_empty && !table_cleared) ? 1 : 0,
                               static_cast<uint32_t*>(d_imp_ovf.ptr), ctr() + FC_RETRY, ctr() + FC_IMP_RECS,
                               ctr() + FC_GROUPS, stream));
    if (table_empty) table_cleared = true;
    DQ_TRY(read_counters(h));
    const uint64_t n_ovf = h[FC_RETRY];
    // group by group: runs out of order (mode 0), keys longer than 15 bytes (mode 1)
    if (any_skip) DQ_HIP(launch_import_global(view(), d_runs, n_runs, max_n, 0, 0, nullptr, nullptr, 0, nullptr, 0, stream));
    if (general) DQ_HIP(launch_import_global(view(), d_runs, n_runs, max_n, 1, 0, nullptr, nullptr, 0, nullptr, 0, stream));
    if (n_ovf) {  // slices whose keys overflowed the image: grow, then insert their records one by one
      // (their records, h[FC_IMP_RECS], bound the keys they add)
      if (debug)
        std::fprintf(stderr, "[dq_freq] import: %llu slices overflowed LDS (%llu records)\n", (unsigned long long)n_ovf,
                     (unsigned long long)h[FC_IMP_RECS]);
      const uint64_t ovf_recs = h[FC_IMP_RECS];
      DQ_TRY(read_counters(h));
      const uint64_t before = capacity;
      DQ_TRY(ensure_capacity(h[FC_GROUPS], ovf_recs + n_ovf * kFreqSliceSlots));
      if (capacity == before) DQ_TRY(grow_to(capacity * 2));
      DQ_HIP(launch_import_global(view(), d_runs, n_runs, max_n, 2, rb, d_start, d_end, n_slices,
                                  static_cast<const uint32_t*>(d_imp_ovf.ptr), n_ovf, stream));
    }
    DQ_TRY(check_overflow());
    if (table_empty && n_ovf == 0 && !any_skip && !general) {
      dev_hist_valid = true;
      smax_valid = true;
    }
    d_imp_bounds.release();
    return DQ_OK;
  }

  dq_status check_overflow() {
    unsigned long long h[FC_COUNT];
    DQ_TRY(read_counters(h));
    const unsigned int ov = (unsigned int)h[FC_OVERFLOW];
    if (ov & kFreqWaitTimeout) return fail(DQ_ERR_DEVICE, "frequency table: a slot publish wait timed out (internal)");
    if (ov & 4u) return fail(DQ_ERR_UNSUPPORTED, "combined grouping key longer than 64 bytes");
    if (ov) return fail(DQ_ERR_DEVICE, "frequency table overflow (internal sizing error)");
    return DQ_OK;
  }
};

// At most this many groups expected: the per-workgroup LDS pre-aggregation of the atomic path
// (dq_freq_insert_kernel, 1024 LDS slots) absorbs nearly every row, which beats staging + sorting.
static const int64_t kFreqFewGroups = 512;
static const int kFreqFewGroupBlocks = 1024;  // insert grid of the few-groups launch (4 per CU: measured best of 128..4096)

extern "C" dq_status dq_freq_create(dq_ctx* ctx, const int32_t* key_columns, int n_keys,
                                    const int32_t* column_types, int n_columns, int flags, dq_freq** out) {
  if (!out) return fail(DQ_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!ctx || !key_columns || !column_types || n_columns <= 0) return fail(DQ_ERR_INVALID, "NULL argument");
  if (n_keys < 1) return fail(DQ_ERR_INVALID, "at least one grouping column is required");
  if (n_keys > kMaxKeyCols) return fail(DQ_ERR_UNSUPPORTED, "too many grouping columns");
  if ((flags & DQ_FREQ_NULL_AS_KEY) && n_keys != 1)
    return fail(DQ_ERR_INVALID, "DQ_FREQ_NULL_AS_KEY needs exactly one grouping column");
  if ((flags & DQ_FREQ_FEW_ONLY) && n_keys != 1)
    return fail(DQ_ERR_INVALID, "DQ_FREQ_FEW_ONLY needs exactly one grouping column");
  if (flags & ~(DQ_FREQ_NULL_AS_KEY | DQ_FREQ_FEW_ONLY)) return fail(DQ_ERR_INVALID, "unknown flag");
  for (int c = 0; c < n_columns; ++c)
    if (!valid_type(column_types[c])) return fail(DQ_ERR_INVALID, "invalid column type");
  DQ_HIP(hipSetDevice(ctx->device));
  dq_freq* f = new dq_freq();
  f->ctx = ctx;
  f->flags = flags;
  f->col_types.assign(column_types, column_types + n_columns);
  f->col_used.assign(n_columns, false);
  f->ks.n_keys = n_keys;
  f->ks.null_as_key = (flags & DQ_FREQ_NULL_AS_KEY) ? 1 : 0;
  if (flags & DQ_FREQ_FEW_ONLY) {
    f->few_only = true;
    f->sorted_path = false;
    f->few_groups = kFreqFewGroups;
  }
  for (int i = 0; i < n_keys; ++i) {
    if (key_columns[i] < 0 || key_columns[i] >= n_columns) {
      delete f;
      return fail(DQ_ERR_INVALID, "grouping column out of range");
    }
    if (is_decimal(column_types[key_columns[i]])) {  // (no key encoding of decimals: DESIGN.md §7)
      delete f;
      return fail(DQ_ERR_UNSUPPORTED, "grouping column " + std::to_string(key_columns[i]) + " is a " +
                                          decimal_name(column_types[key_columns[i]]) +
                                          " column: decimal keys are not on the GPU path");
    }
    f->ks.key_cols[i] = key_columns[i];
    f->col_used[key_columns[i]] = true;
    f->has_utf8 = f->has_utf8 || column_types[key_columns[i]] == DQ_T_UTF8;
  }
  f->resize_stage(n_columns);
  f->h_cols.resize(n_columns);
  if (const char* e = std::getenv("DQ_FREQ_SUBBATCH_ROWS")) {  // test knob: exercise sub-batching
    const long long v = std::atoll(e);
    if (v >= 8) f->sub_rows = v & ~7ll;
  }
  if (const char* e = std::getenv("DQ_FREQ_PATH"))  // test knob: "atomic" = per-row table inserts only
    f->sorted_path = std::strcmp(e, "atomic") != 0;
  if (const char* e = std::getenv("DQ_FREQ_DEBUG")) f->debug = e[0] == '1';
  if (const char* e = std::getenv("DQ_FREQ_PART")) f->part_path = e[0] != '0';  // test knob
  if (const char* e = std::getenv("DQ_FREQ_PACK")) f->pack_default = f->pack_keys = e[0] != '0';  // test / A-B knob
  if (const char* e = std::getenv("DQ_FREQ_COMPACT")) f->compact_enabled = e[0] != '0';  // A-B knob
  if (const char* e = std::getenv("DQ_FREQ_HASHED")) f->hashed_enabled = e[0] != '0';  // A-B / test knob
  if (const char* e = std::getenv("DQ_FREQ_UUID")) f->uuid_enabled = e[0] != '0';  // A-B / test knob
  if (const char* e = std::getenv("DQ_FREQ_SMALL")) f->small_path = e[0] != '0';  // test / A-B knob
  if (const char* e = std::getenv("DQ_FREQ_PART_LOAD")) {  // tuning knob
    const double v = std::atof(e);
    if (v >= 0.1 && v <= 0.95) f->part_load = v;
  }
  if (const char* e = std::getenv("DQ_FREQ_PART_SLOTS")) {  // test knob (a power of two >= 2^16)
    const long long v = std::atoll(e);
    if (v >= (1ll << 16) && (v & (v - 1)) == 0) f->part_slots = (uint64_t)v;
  }
  if (const char* e = std::getenv("DQ_FREQ_PART_MIN")) {                        // test knob
    const long long v = std::atoll(e);
    if (v >= 1) f->part_min = (uint64_t)v;
  }
  if (const char* e = std::getenv("DQ_FREQ_STAGE_BUDGET")) {  // test knob: aggregate early
    const long long v = std::atoll(e);
    if (v >= 1) f->stage_budget = (uint64_t)v;
  }
  dq_status s;
  hipError_t e = StreamPool::get().acquire(ctx->device, &f->stream);
  if (e != hipSuccess) {
    delete f;
    return fail(DQ_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  if ((s = f->d_ctr.ensure(FC_COUNT * sizeof(unsigned long long))) != DQ_OK ||
      (s = f->d_heap.ensure(1u << 20)) != DQ_OK ||
      (s = f->d_cols.ensure(n_columns * sizeof(DevColumn))) != DQ_OK ||
      (s = f->d_hist.ensure(kFreqHist * sizeof(unsigned long long))) != DQ_OK ||
      (s = f->d_sketch.ensure(kHllM * sizeof(uint32_t))) != DQ_OK ||
      (s = dq_freq_reset(f)) != DQ_OK) {
    delete f;
    return s;
  }
  *out = f;
  return DQ_OK;
}


extern "C" dq_status dq_freq_expect_groups(dq_freq* f, int64_t groups) {
  if (!f || groups < 0) return fail(DQ_ERR_INVALID, "bad argument");
  if (groups <= kFreqFewGroups) {
    f->sorted_path = false;
    // each insert launch may add as many groups as it has rows, so the table is sized for the
    // launch: short launches keep a few-group table small (fast to clear and to scan)
    f->sub_rows = std::min<int64_t>(f->sub_rows, (int64_t)1 << 22);
    f->few_groups = std::max<int64_t>(1, groups);
  }
  return DQ_OK;
}

extern "C" dq_status dq_freq_reserve(dq_freq* f, int64_t rows) {
  if (!f || rows < 0) return fail(DQ_ERR_INVALID, "bad argument");
  if (!f->sorted_path || rows == 0) return DQ_OK;
  DQ_HIP(hipSetDevice(f->ctx->device));
  const uint64_t r = (uint64_t)std::min<int64_t>(rows, (int64_t)f->stage_budget);
  f->reserve_rows = r;
  if (f->part_path && r >= f->part_min) return DQ_OK;  // region staging: regions are sized at the first batch
  return f->reserve_stage(r, 1);
}

extern "C" dq_status dq_freq_destroy(dq_freq* f) {
  delete f;
  return DQ_OK;
}

extern "C" dq_status dq_freq_reset(dq_freq* f) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  f->invalidate();
  DQ_HIP(hipSetDevice(f->ctx->device));
  const uint64_t cap = 1u << 16;
  DQ_TRY(f->d_slots.ensure(cap * sizeof(FreqSlot)));
  f->capacity = std::min<uint64_t>(f->d_slots.cap / sizeof(FreqSlot), cap);
  while (f->capacity & (f->capacity - 1)) f->capacity &= f->capacity - 1;
  DQ_HIP(hipMemsetAsync(f->d_slots.ptr, 0, f->capacity * sizeof(FreqSlot), f->stream));
  DQ_HIP(hipMemsetAsync(f->d_ctr.ptr, 0, FC_COUNT * sizeof(unsigned long long), f->stream));
  DQ_HIP(hipMemsetAsync(f->d_sketch.ptr, 0, kHllM * sizeof(uint32_t), f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  f->num_rows = 0;
  f->rows_settled = 0;  // (FC_SELECTED was cleared with the counters; the filter itself stays)
  f->rows_pending = false;
  f->staged = 0;
  f->compact = false;
  f->table_cleared = true;
  f->hash_keys = false;
  f->region_hashed = false;
  f->uuid_probed = false;
  f->wide_keys = 0;
  f->region_wide = 0;
  f->region_staged = false;
  f->region_packed = false;
  f->pack_keys = f->pack_default;
  f->pack_probed = false;
  f->len_probed = false;
  f->region_rows = 0;
  f->d_part1.release();
  f->d_rows.release();
  f->d_povf.release();
  return DQ_OK;
}

extern "C" dq_status dq_freq_set_filter(dq_freq* f, const dq_predicate* where) {
  if (!f || !where) return fail(DQ_ERR_INVALID, "NULL argument");
  if (f->ks.null_as_key)
    return fail(DQ_ERR_UNSUPPORTED, "DQ_FREQ_NULL_AS_KEY: a Histogram table groups its invalid rows, so a row the "
                                    "filter drops cannot be told from a NULL key by validity (no filter on such a table)");
  Program prog;
  DQ_TRY(validate_predicate(*where, f->col_types.data(), (int)f->col_types.size(), &prog));
  DQ_HIP(hipSetDevice(f->ctx->device));
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  if (f->num_rows != 0 || f->staged != 0 || h[FC_GROUPS] != 0 || h[FC_SELECTED] != 0)
    return fail(DQ_ERR_STATE, "dq_freq_set_filter: the table already holds rows or groups (a filter is set on an empty table)");
  // the program's tables, laid out as a plan's (ProgramTables): one program, its pool, one match
  // task per LIKE / RLIKE
  std::vector<MatchTask> tasks;
  std::vector<std::string> keys;
  std::vector<uint32_t> offsets;
  std::vector<uint8_t> images;
  uint32_t lds = 0;
  ProgramTables tables{{}, {}, false, tasks, keys, offsets, images, lds};
  const PredProgram pp = tables.add(prog);
  const std::vector<PredInsn>& insns = tables.insns;
  std::string pool = tables.pool;
  pool.append(8, '\0');
  const bool cast = tables.cast;
  auto upload = [&](DevBuf& buf, const void* src, size_t bytes) -> dq_status {
    if (bytes == 0) return DQ_OK;
    DQ_TRY(buf.ensure(bytes));
    DQ_HIP(hipMemcpy(buf.ptr, src, bytes, hipMemcpyHostToDevice));
    return DQ_OK;
  };
  DQ_TRY(upload(f->d_fprog, &pp, sizeof(pp)));
  DQ_TRY(upload(f->d_finsns, insns.data(), insns.size() * sizeof(PredInsn)));
  DQ_TRY(upload(f->d_fpool, pool.data(), pool.size()));
  DQ_TRY(upload(f->d_fmatch, tasks.data(), tasks.size() * sizeof(MatchTask)));
  DQ_TRY(upload(f->d_fdfas, images.data(), images.size()));
  DQ_TRY(f->d_fcols.ensure(f->col_types.size() * sizeof(DevColumn)));
  for (int c : prog.columns) f->col_used[c] = true;
  f->filter_matches = (int)tasks.size();
  f->filter_lds = lds;
  f->filter_cast = cast;
  f->filtered = true;
  return DQ_OK;
}

// The filter over the prepared batch (h_cols): evaluate, fold into the first key column's validity,
// count the selected rows on the device; h_cols[first key].validity then names the folded bitmap.
dq_status dq_freq::apply_filter(int n_columns, int64_t n_rows) {
  const int64_t wpm = ((n_rows + 63) >> 6) + 1;
  const size_t words = (size_t)wpm * sizeof(uint64_t);
  // Every path of dq_freq_consume reads the counters after its last kernel that reads the folded
  // bitmap, so the stream is idle here and the buffers may be regrown.  rows_pending still set means
  // that the previous consume failed midway: its kernels may be running, so the stream drains
  // before an old block goes back to the pool.
  if (rows_pending && (d_fwords.cap < 2 * words || d_fvalid.cap < words || d_fmatch_words.cap < words * filter_matches))
    DQ_HIP(hipStreamSynchronize(stream));
  DQ_TRY(d_fwords.ensure(2 * words));
  DQ_TRY(d_fvalid.ensure(words));
  // (the descriptors the filter reads, before the fold: its own copies on both sides, the paths
  // below rewrite h_cols and d_cols)
  filter_cols = h_cols;
  DQ_HIP(hipMemcpyAsync(d_fcols.ptr, filter_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice, stream));
  const DevColumn* dcols = static_cast<const DevColumn*>(d_fcols.ptr);
  if (filter_matches > 0) {
    DQ_TRY(d_fmatch_words.ensure((size_t)wpm * filter_matches * sizeof(uint64_t)));
    DQ_HIP(launch_match_mask(static_cast<const MatchTask*>(d_fmatch.ptr), filter_matches, dcols,
                             static_cast<const uint8_t*>(d_fdfas.ptr), filter_lds, n_rows,
                             static_cast<uint64_t*>(d_fmatch_words.ptr), wpm, stream));
  }
  DQ_HIP(launch_predicates(static_cast<const PredProgram*>(d_fprog.ptr), 1, static_cast<const PredInsn*>(d_finsns.ptr),
                           static_cast<const uint8_t*>(d_fpool.ptr), dcols, n_rows, static_cast<uint64_t*>(d_fwords.ptr),
                           wpm, filter_cast, stream, static_cast<const uint64_t*>(d_fmatch_words.ptr)));
  DevColumn& key = h_cols[ks.key_cols[0]];
  DQ_HIP(launch_freq_filter(static_cast<const uint64_t*>(d_fwords.ptr), key.validity, n_rows,
                            static_cast<uint64_t*>(d_fvalid.ptr), ctr() + FC_SELECTED, stream));
  key.validity = static_cast<const uint8_t*>(d_fvalid.ptr);
  rows_pending = true;
  return DQ_OK;
}

static int key_width(int t) {
  switch (t) {
    case DQ_T_BOOL: case DQ_T_INT8: return 1;
    case DQ_T_INT16: return 2;
    case DQ_T_INT32: case DQ_T_FLOAT32: return 4;
    default: return 8;
  }
}

extern "C" dq_status dq_freq_consume(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  if (n_columns != (int)f->col_types.size()) return fail(DQ_ERR_INVALID, "column count differs from the table");
  if (n_rows < 0) return fail(DQ_ERR_INVALID, "negative n_rows");
  if (n_rows == 0) return DQ_OK;
  if (f->few_failed) return fail(DQ_ERR_SPACE, "DQ_FREQ_FEW_ONLY: the column has more groups than the few-groups path holds");
  DQ_HIP(hipSetDevice(f->ctx->device));
  f->invalidate();
  for (int c = 0; c < n_columns; ++c) {
    std::memset(&f->h_cols[c], 0, sizeof(DevColumn));
    if (f->col_used[c]) DQ_TRY(prepare_column(f, c, columns[c], n_rows, &f->h_cols[c]));
  }
  const int64_t rows_before = f->num_rows;
  if (f->filtered) DQ_TRY(f->apply_filter(n_columns, n_rows));  // (counts the selected rows itself)
  else f->num_rows += n_rows;
  if (f->sorted_path && f->part_path &&
      std::max<uint64_t>((uint64_t)n_rows, f->reserve_rows) >= f->part_min) {
    // large stagings: records go straight into their level-1 regions (partition path)
    DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                          f->stream));
    bool ok = false;
    DQ_TRY(f->stage_regions(n_rows, ok));
    if (ok) {
      f->host_tmp.clear();
      if (f->staged >= f->stage_budget) DQ_TRY(f->materialize());
      return DQ_OK;
    }
  } else if (f->sorted_path) {
    // keys of at most 15 bytes take the sorted-bucket path: stage now, aggregate when read
    if (f->region_staged) DQ_TRY(f->materialize());
    DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                          f->stream));
    // optimistic: stage every row as a <= 15-byte inline record; a longer key (possible only for
    // strings or several columns) makes the stage kernel raise FC_MAXLEN, and the whole batch is
    // then rolled back (cursor reset) and grouped on the general path below -- no length pre-pass
    unsigned long long h[FC_COUNT];
    DQ_TRY(f->reserve_stage((uint64_t)n_rows, 2));
    const unsigned long long staged_before = f->staged;
    DQ_HIP(hipMemsetAsync(f->ctr() + FC_MAXLEN, 0, sizeof(unsigned long long), f->stream));
    DQ_HIP(launch_freq_stage(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows,
                             static_cast<FreqRec*>(f->d_stage.ptr),
                             f->ctr() + FC_STAGED, static_cast<uint32_t*>(f->d_sketch.ptr), f->ctr() + FC_MAXLEN,
                             f->stream));
    DQ_TRY(f->read_counters(h));
    if (h[FC_MAXLEN] <= 15) {
      f->staged = h[FC_STAGED];
      f->host_tmp.clear();
      if (f->staged >= f->stage_budget) DQ_TRY(f->materialize());
      return DQ_OK;
    }
    f->staged = staged_before;  // drop this batch's records
    DQ_HIP(hipMemcpyAsync(f->ctr() + FC_STAGED, &f->staged, sizeof(unsigned long long), hipMemcpyHostToDevice,
                          f->stream));
    DQ_HIP(hipStreamSynchronize(f->stream));
  }
  // (the batches staged before this one are aggregated first; the fused counts of that aggregation
  // do not see the rows inserted below)
  DQ_TRY(f->materialize_for_write());
  if (f->few_groups > 0 && f->ks.n_keys == 1 && f->small_path) {
    // Few groups of one key column (the profiler's low-cardinality histograms): per-workgroup LDS
    // counts, staging lists, one merge (dq_freq_small_kernel).  A key longer than 15 bytes or
    // more keys than an LDS table holds: nothing is merged, and the batch takes the paths below.
    unsigned long long h0[FC_COUNT];
    DQ_TRY(f->read_counters(h0));
    DQ_TRY(f->ensure_capacity(h0[FC_GROUPS], (uint64_t)kFreqSmallSlots));
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2 * (int64_t)cus, n_rows / 4096));
    const size_t per = (size_t)blocks * kFreqSmallSlots;
    DQ_TRY(f->d_small.ensure(per * (8 + 8 + 4) + (size_t)blocks * 4 + 8));
    uint8_t* p = static_cast<uint8_t*>(f->d_small.ptr);
    unsigned long long* k0 = reinterpret_cast<unsigned long long*>(p);
    unsigned long long* k1 = k0 + per;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(k1 + per);
    uint32_t* nused = cnt + per;
    unsigned int* bad = reinterpret_cast<unsigned int*>(nused + blocks);
    DQ_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned int), f->stream));
    DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                          f->stream));
    const bool str = f->col_types[f->ks.key_cols[0]] == DQ_T_UTF8;
    DQ_HIP(launch_freq_small(f->ks, str, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows, blocks, k0, k1, cnt,
                             nused, bad, f->view(), f->stream));
    unsigned int hbad = 0;
    DQ_HIP(hipMemcpyAsync(&hbad, bad, sizeof(unsigned int), hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipStreamSynchronize(f->stream));
    if (!hbad) {
      ++f->diag_small_runs;
      DQ_TRY(f->check_overflow());
      f->host_tmp.clear();
      return DQ_OK;
    }
  }
  if (f->few_only) {  // (nothing of this batch was merged)
    f->few_failed = true;
    DQ_TRY(f->settle_rows());
    f->num_rows = rows_before;
    return fail(DQ_ERR_SPACE, "DQ_FREQ_FEW_ONLY: the column has more groups than the few-groups path holds");
  }
  if (f->few_groups > 0 && n_rows > f->sub_rows) {
    // Few groups expected (the profiler's low-cardinality histograms): one launch over the whole
    // batch into a table sized for 64x the hint, instead of per-sub-batch sizing with a host
    // round trip each.  Only from an empty table, and checked: if the hint was wrong (a slot
    // run or the key heap overflowed), the table is cleared and the batch takes the sized path.
    unsigned long long h0[FC_COUNT];
    DQ_TRY(f->read_counters(h0));
    if (h0[FC_GROUPS] == 0 && h0[FC_HEAP_USED] == 0 && h0[FC_OVERFLOW] == 0) {
      const uint64_t room = std::max<uint64_t>(65536, 64 * (uint64_t)f->few_groups);
      DQ_TRY(f->ensure_capacity(0, room));
      if (f->has_utf8 || f->ks.n_keys > 1) DQ_TRY(f->ensure_heap(0, (uint64_t)1 << 20));
      DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                            f->stream));
      // few blocks: every block flushes its (few) LDS groups into the same global slots with
      // device-scope atomics at the end, so the flush contention grows with the block count
      static const int few_blocks = [] {
        const char* e = std::getenv("DQ_FREQ_FEW_BLOCKS");  // test knob
        return e ? std::max(1, std::atoi(e)) : kFreqFewGroupBlocks;
      }();
      DQ_HIP(launch_freq_insert(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows, f->view(), f->stream,
                                few_blocks));
      unsigned long long h[FC_COUNT];
      DQ_TRY(f->read_counters(h));
      if (h[FC_OVERFLOW] == 0) {
        f->host_tmp.clear();
        return DQ_OK;
      }
      if (h[FC_OVERFLOW] & kFreqWaitTimeout) return f->check_overflow();  // a failure, not a sizing miss
      DQ_HIP(hipMemsetAsync(f->d_slots.ptr, 0, f->capacity * sizeof(FreqSlot), f->stream));
      DQ_HIP(hipMemsetAsync(f->ctr() + FC_GROUPS, 0, 3 * sizeof(unsigned long long), f->stream));  // + heap, overflow
    }
  }
  const int64_t kSub = f->sub_rows;
  std::vector<DevColumn> sub(n_columns);
  for (int64_t start = 0; start < n_rows; start += kSub) {
    const int64_t m = std::min(kSub, n_rows - start);
    for (int c = 0; c < n_columns; ++c) {
      sub[c] = f->h_cols[c];
      if (!f->col_used[c]) continue;
      const int t = f->col_types[c];
      if (sub[c].validity) sub[c].validity += start >> 3;
      if (t == DQ_T_UTF8) sub[c].offsets += start;  // offsets stay absolute into the bytes
      else if (t == DQ_T_BOOL) sub[c].values = static_cast<const uint8_t*>(sub[c].values) + (start >> 3);
      else sub[c].values = static_cast<const uint8_t*>(sub[c].values) + start * key_width(t);
    }
    DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, sub.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice, f->stream));
    unsigned long long h[FC_COUNT];
    if (f->has_utf8 || f->ks.n_keys > 1) {
      DQ_HIP(hipMemsetAsync(f->ctr() + FC_NEED, 0, sizeof(unsigned long long), f->stream));
      DQ_HIP(launch_freq_heap_need(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), m, f->ctr() + FC_NEED,
                                   f->ctr() + FC_MAXLEN, f->stream));
    }
    DQ_TRY(f->read_counters(h));  // also fences the descriptor copy before it is rewritten
    DQ_TRY(f->ensure_capacity(h[FC_GROUPS], (uint64_t)m));
    if (f->has_utf8 || f->ks.n_keys > 1) DQ_TRY(f->ensure_heap(h[FC_HEAP_USED], h[FC_NEED]));
    DQ_HIP(launch_freq_insert(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), m, f->view(), f->stream));
  }
  DQ_TRY(f->check_overflow());
  f->host_tmp.clear();
  return DQ_OK;
}

// Metrics from the count-of-counts histogram, summed in ascending count order.
static dq_status freq_hist(dq_freq* f, std::vector<unsigned long long>& hist, std::vector<unsigned long long>& big) {
  DQ_TRY(f->aggregate());
  if (!f->dev_hist_valid) DQ_TRY(f->expand());  // (a compacted table's aggregation counted it)
  if (f->hist_valid) {
    hist = f->hist_cache;
    big = f->big_cache;
    return DQ_OK;
  }
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  const uint64_t groups = h[FC_GROUPS];
  if (!f->dev_hist_valid) {  // (else the partition path's aggregation counted it already)
    DQ_TRY(f->d_big.ensure(std::max<uint64_t>(1, groups) * sizeof(unsigned long long)));
    DQ_HIP(hipMemsetAsync(f->d_hist.ptr, 0, kFreqHist * sizeof(unsigned long long), f->stream));
    DQ_HIP(hipMemsetAsync(f->ctr() + FC_NBIG, 0, sizeof(unsigned long long), f->stream));
    DQ_HIP(launch_freq_hist(f->view(), static_cast<unsigned long long*>(f->d_hist.ptr),
                            static_cast<unsigned long long*>(f->d_big.ptr), f->ctr() + FC_NBIG,
                            std::max<uint64_t>(1, groups), f->stream));
  }
  hist.assign(kFreqHist, 0);
  DQ_HIP(hipMemcpyAsync(hist.data(), f->d_hist.ptr, kFreqHist * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
  DQ_TRY(f->read_counters(h));
  big.assign(h[FC_NBIG], 0);
  if (!big.empty()) {
    DQ_HIP(hipMemcpyAsync(big.data(), f->d_big.ptr, big.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipStreamSynchronize(f->stream));
  }
  std::sort(big.begin(), big.end());
  f->hist_cache = hist;
  f->big_cache = big;
  f->hist_valid = true;
  return DQ_OK;
}

// Metrics from a count-of-counts histogram, summed in ascending count order (deterministic).
static void summary_from_hist(const std::vector<unsigned long long>& hist, const std::vector<unsigned long long>& big,
                              int64_t num_rows, dq_freq_summary* out) {
  std::memset(out, 0, sizeof(*out));
  out->num_rows = num_rows;
  const double n = (double)num_rows;
  double entropy = 0.0;
  auto term = [n](double c) { return c == 0.0 ? 0.0 : -(c / n) * std::log(c / n); };  // Entropy.scala:32-38
  for (size_t c = 1; c < hist.size(); ++c) {
    if (!hist[c]) continue;
    out->num_groups += (int64_t)hist[c];
    out->grouped_rows += (int64_t)hist[c] * (int64_t)c;
    entropy += (double)hist[c] * term((double)c);
  }
  for (unsigned long long c : big) {
    out->num_groups += 1;
    out->grouped_rows += (int64_t)c;
    entropy += term((double)c);
  }
  out->num_unique = hist.size() > 1 ? (int64_t)hist[1] : 0;
  out->entropy = entropy;
}

extern "C" dq_status dq_diag_freq_test_flags(dq_freq* f, int32_t flags) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL argument");
  if (flags & ~kFreqTestNoPublish) return fail(DQ_ERR_INVALID, "unknown test flag");
  f->test_no_publish = (flags & kFreqTestNoPublish) != 0;
  return DQ_OK;
}

extern "C" dq_status dq_diag_freq_paths(dq_freq* f, int64_t* out) {
  if (!f || !out) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->aggregate());
  out[0] = (int64_t)f->capacity;
  out[1] = (int64_t)f->diag_part_runs;
  out[2] = f->diag_part_bits;
  out[3] = (int64_t)f->diag_sort_records;
  out[4] = (int64_t)f->diag_packed_runs;
  out[5] = (int64_t)f->diag_small_runs;
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  out[6] = (int64_t)((h[FC_OVERFLOW] & kFreqWaitTimeout) != 0);
  out[7] = (int64_t)f->diag_import_coarse;
  out[8] = (int64_t)f->diag_import_skipped;
  out[9] = (int64_t)f->diag_hashed_runs;
  out[10] = (int64_t)f->diag_hashed_inserts;
  out[11] = f->compact ? 1 : 0;
  out[12] = (int64_t)f->diag_uuid_runs;
  out[13] = (int64_t)f->diag_raw16_runs;
  out[14] = (int64_t)f->diag_rollbacks;
  out[15] = (int64_t)f->diag_materialized_for_format;
  out[16] = (int64_t)h[FC_HEAP_USED];  // (read above: the key heap's cursor)
  return DQ_OK;
}

extern "C" dq_status dq_freq_get_summary(dq_freq* f, dq_freq_summary* out) {
  if (!f || !out) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  std::vector<unsigned long long> hist, big;
  DQ_TRY(freq_hist(f, hist, big));
  DQ_TRY(f->settle_rows());
  summary_from_hist(hist, big, f->num_rows, out);
  return DQ_OK;
}

static const unsigned long long kCtrlHeap = 1ull << 30;
static const unsigned long long kCtrlLen = (1ull << 24) - 1;

// Export groups with count >= min_count to host arrays (order unspecified).
static dq_status freq_export_raw(dq_freq* f, unsigned long long min_count, uint64_t expect,
                                 std::vector<unsigned long long>& ctrl, std::vector<unsigned long long>& cnt,
                                 std::vector<unsigned long long>& k0, std::vector<unsigned long long>& k1,
                                 std::vector<uint8_t>& heap) {
  DQ_TRY(f->aggregate());
  const uint64_t cap = std::max<uint64_t>(1, expect);
  DQ_TRY(f->d_out.ensure(cap * 4 * sizeof(unsigned long long)));
  unsigned long long* base = static_cast<unsigned long long*>(f->d_out.ptr);
  FreqOut out{base, base + cap, base + 2 * cap, base + 3 * cap, f->ctr() + FC_EXPORT_N, cap};
  DQ_HIP(hipMemsetAsync(f->ctr() + FC_EXPORT_N, 0, sizeof(unsigned long long), f->stream));
  const uint32_t* smax = f->smax_valid ? static_cast<const uint32_t*>(f->d_smax.ptr) : nullptr;
  if (f->compact)  // the occupied slots only, slice by slice
    DQ_HIP(launch_freq_export_compact(f->cmeta(), f->capacity >> kFreqSliceLog, min_count, out, smax, f->stream));
  else
    DQ_HIP(launch_freq_export(f->view(), min_count, out, f->stream, smax));
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  const uint64_t n = std::min<uint64_t>(h[FC_EXPORT_N], cap);
  ctrl.resize(n);
  cnt.resize(n);
  k0.resize(n);
  k1.resize(n);
  if (n) {
    DQ_HIP(hipMemcpyAsync(ctrl.data(), out.ctrl, n * 8, hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipMemcpyAsync(cnt.data(), out.count, n * 8, hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipMemcpyAsync(k0.data(), out.k0, n * 8, hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipMemcpyAsync(k1.data(), out.k1, n * 8, hipMemcpyDeviceToHost, f->stream));
  }
  DQ_HIP(hipStreamSynchronize(f->stream));
  // the exported groups' heap keys only: gathered on the device (a hashed-path table's heap holds
  // every row's key bytes -- tens of GB -- of which a top-N export needs a few KB)
  std::vector<unsigned long long> off(n, 0ull);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (!(ctrl[i] & kCtrlHeap)) continue;
    off[i] = total;
    total += ((ctrl[i] & kCtrlLen) + 7ull) & ~7ull;
  }
  heap.assign(total, 0);
  if (total) {
    DevBuf tmp;
    DQ_TRY(tmp.ensure(n * 8 + total));
    unsigned long long* d_off = static_cast<unsigned long long*>(tmp.ptr);
    uint8_t* d_dst = static_cast<uint8_t*>(tmp.ptr) + n * 8;
    DQ_HIP(hipMemcpyAsync(d_off, off.data(), n * 8, hipMemcpyHostToDevice, f->stream));
    DQ_HIP(launch_freq_gather_keys(static_cast<const uint8_t*>(f->d_heap.ptr), out.ctrl, out.k0, d_off, n, d_dst,
                                   f->stream));
    DQ_HIP(hipMemcpyAsync(heap.data(), d_dst, total, hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipStreamSynchronize(f->stream));
    for (uint64_t i = 0; i < n; ++i)
      if (ctrl[i] & kCtrlHeap) k0[i] = off[i];  // (key_bytes_of reads heap + k0)
  }
  return DQ_OK;
}


static void key_bytes_of(unsigned long long ctrl, unsigned long long k0, unsigned long long k1,
                         const std::vector<uint8_t>& heap, std::string* out) {
  const uint32_t len = (uint32_t)(ctrl & kCtrlLen);
  out->resize(len);
  if (ctrl & kCtrlHeap) {
    std::memcpy(&(*out)[0], heap.data() + k0, len);
  } else {
    for (uint32_t i = 0; i < len; ++i) (*out)[i] = (char)((i < 8 ? k0 >> (8 * i) : k1 >> (8 * (i - 8))) & 0xff);
  }
}

extern "C" dq_status dq_freq_size(dq_freq* f, int64_t* n_groups, int64_t* key_bytes) {
  if (!f || !n_groups || !key_bytes) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->aggregate());
  std::vector<unsigned long long> ctrl, cnt, k0, k1;
  std::vector<uint8_t> heap;
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  DQ_TRY(freq_export_raw(f, 0, h[FC_GROUPS], ctrl, cnt, k0, k1, heap));
  int64_t bytes = 0;
  for (unsigned long long c : ctrl) bytes += (int64_t)(c & kCtrlLen);
  *n_groups = (int64_t)ctrl.size();
  *key_bytes = bytes;
  return DQ_OK;
}

static dq_status fill_groups(const std::vector<size_t>& order, const std::vector<unsigned long long>& ctrl,
                             const std::vector<unsigned long long>& cnt, const std::vector<unsigned long long>& k0,
                             const std::vector<unsigned long long>& k1, const std::vector<uint8_t>& heap,
                             dq_freq_group* groups, uint8_t* key_bytes, int64_t key_cap) {
  int64_t off = 0;
  std::string key;
  for (size_t j = 0; j < order.size(); ++j) {
    const size_t i = order[j];
    key_bytes_of(ctrl[i], k0[i], k1[i], heap, &key);
    if (off + (int64_t)key.size() > key_cap) return fail(DQ_ERR_SPACE, "key byte buffer too small");
    if (!key.empty()) std::memcpy(key_bytes + off, key.data(), key.size());
    groups[j].count = (int64_t)cnt[i];
    groups[j].key_offset = off;
    groups[j].key_len = (int32_t)key.size();
    groups[j].reserved = 0;
    off += (int64_t)key.size();
  }
  return DQ_OK;
}

extern "C" dq_status dq_freq_export(dq_freq* f, dq_freq_group* groups, int64_t max_groups, uint8_t* key_bytes,
                                    int64_t key_cap, int64_t* n_out) {
  if (!f || !n_out || (max_groups > 0 && !groups)) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->aggregate());
  std::vector<unsigned long long> ctrl, cnt, k0, k1;
  std::vector<uint8_t> heap;
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  DQ_TRY(freq_export_raw(f, 0, h[FC_GROUPS], ctrl, cnt, k0, k1, heap));
  if ((int64_t)ctrl.size() > max_groups) return fail(DQ_ERR_SPACE, "group buffer too small");
  std::vector<size_t> order(ctrl.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  DQ_TRY(fill_groups(order, ctrl, cnt, k0, k1, heap, groups, key_bytes, key_cap));
  *n_out = (int64_t)ctrl.size();
  return DQ_OK;
}

// The flat export on the device (slot order): counts, (n + 1) byte offsets and the key bytes,
// kept in f->d_flat / d_flat_bytes until the table changes or dq_freq_export_flat hands them over.
static dq_status freq_flat_build(dq_freq* f) {
  if (f->flat_valid) return DQ_OK;
  DQ_TRY(f->materialize());
  const FreqTable T = f->view();
  const uint64_t nc = freq_flat_chunks(f->capacity);
  const uint64_t sums_c = (nc + 1 + 4095) / 4096;
  DQ_TRY(f->d_flat_aux.ensure((nc + 1 + sums_c) * sizeof(unsigned long long)));
  unsigned long long* chunk = static_cast<unsigned long long*>(f->d_flat_aux.ptr);
  DQ_HIP(launch_freq_flat_count(T, chunk, nc, chunk + nc + 1, f->stream));
  unsigned long long n = 0;
  DQ_HIP(hipMemcpyAsync(&n, chunk + nc, sizeof(n), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  const uint64_t sums_n = (n + 1 + 4095) / 4096;
  DQ_TRY(f->d_flat.ensure((5 * n + 1 + sums_n) * sizeof(unsigned long long)));
  unsigned long long* a = static_cast<unsigned long long*>(f->d_flat.ptr);
  unsigned long long *ctrl = a, *cnt = a + n, *k0 = a + 2 * n, *k1 = a + 3 * n, *offs = a + 4 * n;
  DQ_HIP(launch_freq_flat_fill(T, chunk, nc, n, ctrl, cnt, k0, k1, offs, offs + n + 1, f->stream));
  unsigned long long bytes = 0;
  DQ_HIP(hipMemcpyAsync(&bytes, offs + n, sizeof(bytes), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  DQ_TRY(f->d_flat_bytes.ensure(bytes + 16));
  DQ_HIP(launch_freq_flat_keys(T, ctrl, k0, k1, offs, n, static_cast<uint8_t*>(f->d_flat_bytes.ptr), f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  f->flat_n = n;
  f->flat_bytes = bytes;
  f->flat_valid = true;
  return DQ_OK;
}

extern "C" dq_status dq_freq_export_flat(dq_freq* f, int64_t* counts, int64_t* key_offsets, uint8_t* key_bytes,
                                         int64_t max_groups, int64_t key_cap, int flags, int64_t* n_out,
                                         int64_t* key_bytes_out) {
  if (!f || !n_out || !key_bytes_out) return fail(DQ_ERR_INVALID, "NULL argument");
  if (flags & ~DQ_FLAT_DEVICE) return fail(DQ_ERR_INVALID, "unknown flag");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(freq_flat_build(f));
  const uint64_t n = f->flat_n, bytes = f->flat_bytes;
  *n_out = (int64_t)n;
  *key_bytes_out = (int64_t)bytes;
  if ((int64_t)n > max_groups || (int64_t)bytes > key_cap || !key_offsets || (n && !counts) || (bytes && !key_bytes))
    return fail(DQ_ERR_SPACE, "output buffers too small for the groups");
  const hipMemcpyKind kind = (flags & DQ_FLAT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const unsigned long long* a = static_cast<const unsigned long long*>(f->d_flat.ptr);
  if (n) DQ_HIP(hipMemcpyAsync(counts, a + n, n * 8, kind, f->stream));
  DQ_HIP(hipMemcpyAsync(key_offsets, a + 4 * n, (n + 1) * 8, kind, f->stream));
  if (bytes) DQ_HIP(hipMemcpyAsync(key_bytes, f->d_flat_bytes.ptr, bytes, kind, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  // handed over: the device copy is not kept (it can be as large as the table)
  f->flat_valid = false;
  f->d_flat.release();
  f->d_flat_bytes.release();
  f->d_flat_aux.release();
  return DQ_OK;
}

extern "C" dq_status dq_freq_import_flat(dq_freq* f, const int64_t* counts, const int64_t* key_offsets,
                                         const uint8_t* key_bytes, int64_t n, int64_t num_rows, int flags) {
  if (!f || n < 0 || (n > 0 && (!counts || !key_offsets))) return fail(DQ_ERR_INVALID, "NULL argument");
  if (flags & ~DQ_FLAT_DEVICE) return fail(DQ_ERR_INVALID, "unknown flag");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize_for_write());
  if (n == 0) {
    f->num_rows += num_rows;
    return DQ_OK;
  }
  const bool dev = (flags & DQ_FLAT_DEVICE) != 0;
  std::vector<int64_t> hoff;
  const int64_t* off = key_offsets;
  if (dev) {
    hoff.resize((size_t)n + 1);
    DQ_HIP(hipMemcpyAsync(hoff.data(), key_offsets, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, f->stream));
    DQ_HIP(hipStreamSynchronize(f->stream));
    off = hoff.data();
  }
  // (validated before anything changes: a bad offset array leaves the table as it was)
  if (off[0] < 0) return fail(DQ_ERR_INVALID, "negative key offset");
  uint64_t long_bytes = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = off[i + 1] - off[i];
    if (len < 0 || len > (1 << 23)) return fail(DQ_ERR_INVALID, "bad key length");
    if (len > 16) long_bytes += ((uint64_t)len + 7) & ~7ull;
  }
  if (off[n] > 0 && !key_bytes) return fail(DQ_ERR_INVALID, "NULL key bytes");
  const long long *d_cnt, *d_off;
  const uint8_t* d_bytes;
  if (dev) {
    d_cnt = reinterpret_cast<const long long*>(counts);
    d_off = reinterpret_cast<const long long*>(key_offsets);
    d_bytes = key_bytes;
  } else {
    const size_t a = (size_t)n * 8, b = ((size_t)n + 1) * 8, c = (size_t)off[n];
    DQ_TRY(f->d_in.ensure(a + b + c + 16));
    uint8_t* base = static_cast<uint8_t*>(f->d_in.ptr);
    DQ_HIP(hipMemcpyAsync(base, counts, a, hipMemcpyHostToDevice, f->stream));
    DQ_HIP(hipMemcpyAsync(base + a, key_offsets, b, hipMemcpyHostToDevice, f->stream));
    if (c) DQ_HIP(hipMemcpyAsync(base + a + b, key_bytes, c, hipMemcpyHostToDevice, f->stream));
    d_cnt = reinterpret_cast<const long long*>(base);
    d_off = reinterpret_cast<const long long*>(base + a);
    d_bytes = base + a + b;
  }
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  DQ_TRY(f->ensure_capacity(h[FC_GROUPS], (uint64_t)n));
  DQ_TRY(f->ensure_heap(h[FC_HEAP_USED], long_bytes));
  DQ_HIP(launch_freq_import_flat(f->view(), d_cnt, d_off, d_bytes, (uint64_t)n, f->stream));
  DQ_TRY(f->check_overflow());
  // numRows moves only with the groups: a failed reservation or import leaves both as they were
  f->num_rows += num_rows;
  return DQ_OK;
}

extern "C" dq_status dq_freq_top(dq_freq* f, int n, dq_freq_group* groups, int64_t max_groups, uint8_t* key_bytes,
                                 int64_t key_cap, int64_t* n_out, int64_t* key_bytes_out) {
  if (!f || !n_out || !key_bytes_out) return fail(DQ_ERR_INVALID, "NULL argument");
  *n_out = 0;
  *key_bytes_out = 0;
  if (n <= 0) return DQ_OK;
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->aggregate());
  if (f->top_n != n) {  // (a retry with larger buffers reuses the last result)
    std::vector<unsigned long long> hist, big;
    DQ_TRY(freq_hist(f, hist, big));
    // threshold T: the n-th largest count (1 when there are fewer than n groups)
    unsigned long long threshold = 1, above = 0;
    bool found = false;
    for (size_t i = big.size(); i-- > 0;) {
      if (++above >= (unsigned long long)n) {
        threshold = big[i];
        found = true;
        break;
      }
    }
    for (int c = kFreqHist - 1; !found && c >= 1; --c) {
      above += hist[c];
      if (hist[c] && above >= (unsigned long long)n) {
        threshold = (unsigned long long)c;
        found = true;
      }
    }
    uint64_t expect = 0;
    for (unsigned long long c : big) expect += c >= threshold;
    for (int c = 1; c < kFreqHist; ++c) expect += (unsigned long long)c >= threshold ? hist[c] : 0;
    std::vector<unsigned long long> ctrl, cnt, k0, k1;
    std::vector<uint8_t> heap;
    DQ_TRY(freq_export_raw(f, threshold, expect, ctrl, cnt, k0, k1, heap));
    f->top_cache.resize(ctrl.size());
    for (size_t i = 0; i < ctrl.size(); ++i) {
      f->top_cache[i].first = cnt[i];
      key_bytes_of(ctrl[i], k0[i], k1[i], heap, &f->top_cache[i].second);
    }
    std::sort(f->top_cache.begin(), f->top_cache.end(), [](const std::pair<unsigned long long, std::string>& a,
                                                           const std::pair<unsigned long long, std::string>& b) {
      if (a.first != b.first) return a.first > b.first;
      return a.second < b.second;
    });
    f->top_n = n;
  }
  int64_t total = 0;
  for (const auto& g : f->top_cache) total += (int64_t)g.second.size();
  *n_out = (int64_t)f->top_cache.size();
  *key_bytes_out = total;
  if (*n_out > max_groups || total > key_cap || (*n_out > 0 && !groups) || (total > 0 && !key_bytes))
    return fail(DQ_ERR_SPACE, "output buffers too small for the top groups");
  int64_t off = 0;
  for (size_t j = 0; j < f->top_cache.size(); ++j) {
    const std::string& key = f->top_cache[j].second;
    if (!key.empty()) std::memcpy(key_bytes + off, key.data(), key.size());
    groups[j].count = (int64_t)f->top_cache[j].first;
    groups[j].key_offset = off;
    groups[j].key_len = (int32_t)key.size();
    groups[j].reserved = 0;
    off += (int64_t)key.size();
  }
  return DQ_OK;
}

extern "C" dq_status dq_freq_lookup(dq_freq* f, const uint8_t* key, int64_t key_len, int64_t* count) {
  if (!f || !count || (key_len > 0 && !key)) return fail(DQ_ERR_INVALID, "NULL argument");
  if (key_len < 0 || key_len > (int64_t)kCtrlLen) return fail(DQ_ERR_INVALID, "bad key length");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->aggregate());  // (a compacted table is looked up in its key's slice: no expand)
  DQ_TRY(f->d_in.ensure((size_t)key_len + 16));
  if (key_len) DQ_HIP(hipMemcpyAsync(f->d_in.ptr, key, (size_t)key_len, hipMemcpyHostToDevice, f->stream));
  const FreqCompact cmp = f->compact ? f->cmeta() : FreqCompact{};
  DQ_HIP(launch_freq_lookup(f->view(), static_cast<const uint8_t*>(f->d_in.ptr), (uint32_t)key_len,
                            f->ctr() + FC_EXPORT_N, f->stream, f->compact ? &cmp : nullptr));
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  *count = (int64_t)h[FC_EXPORT_N];
  return DQ_OK;
}

// Row-level outcomes of Uniqueness (include/deequ_amd.h "row-level outcomes"): see dq_freq.hip
// "Row-level probe" and dq_rows.hip.  The table is materialised first and its stream is idle
// (read_counters) before the probe's launch reads the slot image.
extern "C" dq_status dq_freq_probe_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows,
                                        const uint64_t* d_selected, int64_t out_bit_offset, uint64_t* d_value,
                                        uint64_t* d_valid, int64_t* d_counts) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  if (f->ks.null_as_key)
    return fail(DQ_ERR_INVALID, "dq_freq_probe_rows: a DQ_FREQ_NULL_AS_KEY (Histogram) table groups its NULLs, so "
                                "\"count == 1\" there is not Uniqueness's outcome");
  if (n_columns != (int)f->col_types.size()) return fail(DQ_ERR_INVALID, "column count differs from the table");
  if (n_rows < 0 || out_bit_offset < 0) return fail(DQ_ERR_INVALID, "negative n_rows or out_bit_offset");
  if (n_rows == 0) return DQ_OK;
  if (!columns || !d_value || !d_valid) return fail(DQ_ERR_INVALID, "NULL argument");
  if (f->few_failed) return fail(DQ_ERR_SPACE, "DQ_FREQ_FEW_ONLY: the column has more groups than the few-groups path holds");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize());
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  const size_t words = (size_t)((n_rows + 63) >> 6);
  DQ_TRY(f->d_probe.ensure(words * sizeof(uint64_t)));
  uint64_t* unique = static_cast<uint64_t*>(f->d_probe.ptr);
  if (h[FC_GROUPS] == 0) {  // (no group: no key is in the table, and its slot image may not exist yet)
    DQ_HIP(hipMemsetAsync(unique, 0, words * sizeof(uint64_t), f->stream));
    if (d_counts) DQ_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_rows * sizeof(int64_t), f->stream));
  } else {
    for (int c = 0; c < n_columns; ++c) std::memset(&f->h_cols[c], 0, sizeof(DevColumn));
    for (int i = 0; i < f->ks.n_keys; ++i) {  // (the key columns only: a filtered table's other columns are not read)
      const int c = f->ks.key_cols[i];
      DQ_TRY(prepare_column(f, c, columns[c], n_rows, &f->h_cols[c]));
    }
    DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                          f->stream));
    DQ_HIP(launch_freq_probe_rows(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows, f->view(), unique,
                                  reinterpret_cast<long long*>(d_counts), f->stream));
  }
  DQ_HIP(launch_rows_combine(nullptr, unique, d_selected, n_rows, out_bit_offset, d_value, d_valid, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  f->host_tmp.clear();
  return DQ_OK;
}

// Cross-table checks (include/deequ_amd.h "cross-table checks"): dq_freq.hip "Cross-table checks".
// Both calls materialise the table and leave its stream idle (read_counters) before their launch
// reads the slot image; a table without groups has its image cleared first (an aggregation that
// found no key may have left it unwritten), so the kernels run on it as on any other.
static dq_status cross_prepare(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows, const char* who) {
  if (f->ks.null_as_key)
    return fail(DQ_ERR_INVALID, std::string(who) + ": a DQ_FREQ_NULL_AS_KEY (Histogram) table groups its NULLs, so "
                                                   "\"the table holds the key\" is not a join's condition there");
  if (n_columns != (int)f->col_types.size()) return fail(DQ_ERR_INVALID, "column count differs from the table");
  if (f->few_failed) return fail(DQ_ERR_SPACE, "DQ_FREQ_FEW_ONLY: the column has more groups than the few-groups path holds");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize());
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  if (h[FC_GROUPS] == 0) DQ_TRY(f->clear_table());
  for (int c = 0; c < n_columns; ++c) std::memset(&f->h_cols[c], 0, sizeof(DevColumn));
  for (int i = 0; i < f->ks.n_keys; ++i) {  // (the key columns only)
    const int c = f->ks.key_cols[i];
    DQ_TRY(prepare_column(f, c, columns[c], n_rows, &f->h_cols[c]));
  }
  DQ_HIP(hipMemcpyAsync(f->d_cols.ptr, f->h_cols.data(), n_columns * sizeof(DevColumn), hipMemcpyHostToDevice,
                        f->stream));
  return DQ_OK;
}

extern "C" dq_status dq_freq_index_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows,
                                        int64_t row_offset) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  if (n_rows < 0 || row_offset < 0) return fail(DQ_ERR_INVALID, "negative n_rows or row_offset");
  if (n_rows > 0 && !columns) return fail(DQ_ERR_INVALID, "NULL argument");
  if (f->filtered)
    return fail(DQ_ERR_INVALID, "dq_freq_index_rows: a filtered table does not hold the keys of the rows its filter "
                                "dropped, so the batch is not what it was built from");
  DQ_TRY(cross_prepare(f, columns, n_columns, n_rows, "dq_freq_index_rows"));
  if (!f->index_valid) {  // (first call since the table last changed: one entry per slot, all -1)
    DQ_TRY(f->d_row_of_slot.ensure((size_t)f->capacity * sizeof(int64_t)));
    DQ_HIP(hipMemsetAsync(f->d_row_of_slot.ptr, 0xff, (size_t)f->capacity * sizeof(int64_t), f->stream));
    f->index_valid = true;
  }
  DQ_TRY(f->d_match.ensure(dq_freq::kMatchHeadBytes));
  unsigned long long* d_absent = static_cast<unsigned long long*>(f->d_match.ptr);
  DQ_HIP(hipMemsetAsync(d_absent, 0, sizeof(unsigned long long), f->stream));
  DQ_HIP(launch_freq_index_rows(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows, f->view(),
                                static_cast<long long*>(f->d_row_of_slot.ptr), row_offset, d_absent, f->stream));
  unsigned long long absent = 0;
  DQ_HIP(hipMemcpyAsync(&absent, d_absent, sizeof(absent), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  f->host_tmp.clear();
  if (absent != 0) {
    f->drop_index();
    return fail(DQ_ERR_STATE, "dq_freq_index_rows: " + std::to_string(absent) + " rows hold a key the table does not: "
                              "the batch is not what the table was built from");
  }
  return DQ_OK;
}

static dq_status compare_cells(const dq_column& col, int64_t rows, const char* side, int p, celleq::Cells* out) {
  const std::string who = std::string("dq_freq_match_rows: ") + side + " compare column " + std::to_string(p);
  if (!valid_type(col.type)) return fail(DQ_ERR_INVALID, who + " has an invalid type");
  if (!(col.flags & DQ_COL_DEVICE)) return fail(DQ_ERR_INVALID, who + " is not DQ_COL_DEVICE (compare columns are read in place)");
  if (col.length < rows || col.offset < 0) return fail(DQ_ERR_INVALID, who + " is shorter than its table, or its offset is negative");
  if (rows > 0 && !col.values) return fail(DQ_ERR_INVALID, who + " has no values");
  if ((col.type & 0xff) == DQ_T_UTF8 && !col.offsets) return fail(DQ_ERR_INVALID, who + " is utf8 without offsets");
  *out = celleq::Cells{col.validity, col.values, col.offsets, col.type, 0, col.offset};
  return DQ_OK;
}

extern "C" dq_status dq_freq_match_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows,
                                        const uint64_t* d_selected, int64_t out_bit_offset, uint64_t* d_value,
                                        uint64_t* d_valid, const dq_column* a_compare, const dq_column* b_compare,
                                        int n_pairs, int64_t b_rows, int64_t* d_reference_rows,
                                        dq_match_counts* counts) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  if (n_rows < 0 || out_bit_offset < 0 || n_pairs < 0 || b_rows < 0)
    return fail(DQ_ERR_INVALID, "negative n_rows, out_bit_offset, n_pairs or b_rows");
  if (n_pairs > DQ_MATCH_MAX_PAIRS) return fail(DQ_ERR_UNSUPPORTED, "more than 32 compare pairs");
  if (n_pairs > 0 && (!a_compare || !b_compare)) return fail(DQ_ERR_INVALID, "NULL compare columns");
  if (n_rows == 0) return DQ_OK;
  if (!columns || !d_value || !d_valid) return fail(DQ_ERR_INVALID, "NULL argument");
  std::vector<celleq::Cells> cells((size_t)2 * n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    if (a_compare[p].type != b_compare[p].type)
      return fail(DQ_ERR_INVALID, "dq_freq_match_rows: compare pair " + std::to_string(p) + " has two types");
    DQ_TRY(compare_cells(a_compare[p], n_rows, "primary", p, &cells[p]));
    DQ_TRY(compare_cells(b_compare[p], b_rows, "reference", p, &cells[n_pairs + p]));
  }
  const bool follow = n_pairs > 0 || d_reference_rows != nullptr;
  if (follow && !f->index_valid)
    return fail(DQ_ERR_STATE, "dq_freq_match_rows: compare pairs and reference rows need dq_freq_index_rows after the "
                              "table last changed");
  DQ_TRY(cross_prepare(f, columns, n_columns, n_rows, "dq_freq_match_rows"));
  if (follow && !f->index_valid) return fail(DQ_ERR_STATE, "dq_freq_match_rows: the table changed under its row index");
  const size_t words = (size_t)((n_rows + 63) >> 6);
  DQ_TRY(f->d_probe.ensure(words * sizeof(uint64_t)));
  DQ_TRY(f->d_match.ensure(dq_freq::kMatchHeadBytes + cells.size() * sizeof(celleq::Cells)));
  uint8_t* base = static_cast<uint8_t*>(f->d_match.ptr);
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(base) + 1;  // (word 0: the index's counter)
  celleq::Cells* d_cells = reinterpret_cast<celleq::Cells*>(base + dq_freq::kMatchHeadBytes);
  DQ_HIP(hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), f->stream));
  if (n_pairs > 0)
    DQ_HIP(hipMemcpyAsync(d_cells, cells.data(), cells.size() * sizeof(celleq::Cells), hipMemcpyHostToDevice, f->stream));
  uint64_t* matched = static_cast<uint64_t*>(f->d_probe.ptr);
  DQ_HIP(launch_freq_match_rows(f->ks, static_cast<const DevColumn*>(f->d_cols.ptr), n_rows, f->view(), d_selected,
                                follow ? static_cast<const long long*>(f->d_row_of_slot.ptr) : nullptr, b_rows, d_cells,
                                d_cells + n_pairs, n_pairs, matched, reinterpret_cast<long long*>(d_reference_rows),
                                d_counts, f->stream));
  DQ_HIP(launch_rows_combine(nullptr, matched, d_selected, n_rows, out_bit_offset, d_value, d_valid, f->stream));
  unsigned long long got[4] = {0, 0, 0, 0};
  DQ_HIP(hipMemcpyAsync(got, d_counts, sizeof(got), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  f->host_tmp.clear();
  if (counts) {
    counts->matched += (int64_t)got[0];
    counts->key_null += (int64_t)got[1];
    counts->key_absent += (int64_t)got[2];
    counts->cells_differ += (int64_t)got[3];
  }
  return DQ_OK;
}

extern "C" dq_status dq_freq_import(dq_freq* f, const dq_freq_group* groups, int64_t n, const uint8_t* key_bytes,
                                    int64_t num_rows) {
  if (!f || (n > 0 && !groups)) return fail(DQ_ERR_INVALID, "NULL argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize_for_write());
  f->num_rows += num_rows;
  if (n == 0) return DQ_OK;
  // device arrays: ctrl (len | heap flag), count, k0 (inline bytes or offset into the uploaded
  // key bytes), k1, then the key bytes themselves
  std::vector<unsigned long long> ctrl(n), cnt(n), k0(n), k1(n);
  uint64_t long_bytes = 0;
  int64_t total_key = 0;
  for (int64_t i = 0; i < n; ++i) total_key = std::max<int64_t>(total_key, groups[i].key_offset + groups[i].key_len);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t len = groups[i].key_len;
    if (len < 0 || len > (1 << 23)) return fail(DQ_ERR_INVALID, "bad key length");
    const uint8_t* p = key_bytes + groups[i].key_offset;
    cnt[i] = (unsigned long long)groups[i].count;
    if (len <= 16) {
      ctrl[i] = (unsigned long long)len;
      uint64_t a = 0, b = 0;
      for (int j = 0; j < len; ++j) {
        if (j < 8) a |= (uint64_t)p[j] << (8 * j);
        else b |= (uint64_t)p[j] << (8 * (j - 8));
      }
      k0[i] = a;
      k1[i] = b;
    } else {
      ctrl[i] = kCtrlHeap | (unsigned long long)len;
      k0[i] = (unsigned long long)groups[i].key_offset;
      k1[i] = 0;
      long_bytes += ((uint64_t)len + 7) & ~7ull;
    }
  }
  const size_t arr = (size_t)n * 8;
  DQ_TRY(f->d_in.ensure(arr * 4 + (size_t)total_key + 16));
  uint8_t* base = static_cast<uint8_t*>(f->d_in.ptr);
  DQ_HIP(hipMemcpyAsync(base, ctrl.data(), arr, hipMemcpyHostToDevice, f->stream));
  DQ_HIP(hipMemcpyAsync(base + arr, cnt.data(), arr, hipMemcpyHostToDevice, f->stream));
  DQ_HIP(hipMemcpyAsync(base + 2 * arr, k0.data(), arr, hipMemcpyHostToDevice, f->stream));
  DQ_HIP(hipMemcpyAsync(base + 3 * arr, k1.data(), arr, hipMemcpyHostToDevice, f->stream));
  if (total_key) DQ_HIP(hipMemcpyAsync(base + 4 * arr, key_bytes, (size_t)total_key, hipMemcpyHostToDevice, f->stream));
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  DQ_TRY(f->ensure_capacity(h[FC_GROUPS], (uint64_t)n));
  DQ_TRY(f->ensure_heap(h[FC_HEAP_USED], long_bytes));
  FreqIn in{reinterpret_cast<const unsigned long long*>(base), reinterpret_cast<const unsigned long long*>(base + arr),
            reinterpret_cast<const unsigned long long*>(base + 2 * arr),
            reinterpret_cast<const unsigned long long*>(base + 3 * arr), base + 4 * arr, (uint64_t)n, 1};
  DQ_HIP(launch_freq_import(f->view(), in, f->stream));
  return f->check_overflow();
}

extern "C" dq_status dq_freq_merge(dq_freq* dst, dq_freq* src) {
  if (!dst || !src) return fail(DQ_ERR_INVALID, "NULL table");
  if (dst == src) return fail(DQ_ERR_INVALID, "cannot merge a table into itself");
  if (dst->ctx->device != src->ctx->device) return fail(DQ_ERR_INVALID, "tables live on different devices");
  if (dst->ks.n_keys != src->ks.n_keys || dst->ks.null_as_key != src->ks.null_as_key)
    return fail(DQ_ERR_INVALID, "tables group different keys");
  for (int i = 0; i < dst->ks.n_keys; ++i)
    if (dst->col_types[dst->ks.key_cols[i]] != src->col_types[src->ks.key_cols[i]])
      return fail(DQ_ERR_INVALID, "tables group different key types");
  DQ_HIP(hipSetDevice(dst->ctx->device));
  DQ_TRY(src->materialize());
  unsigned long long hs[FC_COUNT];
  DQ_TRY(src->read_counters(hs));  // (also: src's stream is idle before dst's kernels read its table)
  // src's slot array is one run in slice order: every dst slice reads the src slots of its hash
  // range (FrequenciesAndNumRows.sum, GroupingAnalyzers.scala:128-148)
  std::vector<ImportRun> runs(1);
  runs[0] = ImportRun{src->d_slots.ptr, src->capacity, static_cast<const uint8_t*>(src->d_heap.ptr), 2,
                      slice_bits_for(src->capacity), 0, 0};
  if (hs[FC_GROUPS]) DQ_TRY(dst->import_runs(runs, (int64_t)hs[FC_GROUPS], hs[FC_HEAP_USED]));
  else dst->invalidate();  // (defensive: no group changed, and no cached view depends on num_rows)
  dst->num_rows += src->num_rows;
  return DQ_OK;
}

// Distance.categoricalDistance over two device states (Distance.scala:43-87): see dq_freq.hip
// "Distance".  Words of a->d_dist: {max bits, common, a's lo / hi / groups, b's lo / hi / groups}.
extern "C" dq_status dq_freq_linf_distance(dq_freq* a, dq_freq* b, dq_freq_distance* out) {
  if (!a || !b) return fail(DQ_ERR_INVALID, "NULL table");
  if (!out) return fail(DQ_ERR_INVALID, "NULL argument");
  if (a->ctx->device != b->ctx->device) return fail(DQ_ERR_INVALID, "tables live on different devices");
  if (a->ks.n_keys != b->ks.n_keys || a->ks.null_as_key != b->ks.null_as_key)
    return fail(DQ_ERR_INVALID, "tables group different keys");
  for (int i = 0; i < a->ks.n_keys; ++i)
    if (a->col_types[a->ks.key_cols[i]] != b->col_types[b->ks.key_cols[i]])
      return fail(DQ_ERR_INVALID, "tables group different key types");
  DQ_HIP(hipSetDevice(a->ctx->device));
  DQ_TRY(a->materialize());
  if (b != a) DQ_TRY(b->materialize());
  unsigned long long ha[FC_COUNT], hb[FC_COUNT];
  DQ_TRY(a->read_counters(ha));
  DQ_TRY(b->read_counters(hb));  // (also: b's stream is idle before a's kernels read its table)
  DQ_TRY(a->d_dist.ensure(8 * sizeof(unsigned long long)));
  unsigned long long* d = static_cast<unsigned long long*>(a->d_dist.ptr);
  unsigned long long w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  DQ_HIP(hipMemsetAsync(d, 0, sizeof(w), a->stream));
  if (ha[FC_GROUPS]) DQ_HIP(launch_freq_totals(a->view(), d + 2, a->stream));
  if (hb[FC_GROUPS]) DQ_HIP(launch_freq_totals(b->view(), d + 5, a->stream));
  if (ha[FC_GROUPS] || hb[FC_GROUPS]) {
    DQ_HIP(hipMemcpyAsync(w, d, sizeof(w), hipMemcpyDeviceToHost, a->stream));
    DQ_HIP(hipStreamSynchronize(a->stream));
  }
  const unsigned __int128 limit = (unsigned __int128)1 << 53;
  const unsigned __int128 n = ((unsigned __int128)w[3] << 32) + w[2], m = ((unsigned __int128)w[6] << 32) + w[5];
  if (n > limit || m > limit)
    return fail(DQ_ERR_UNSUPPORTED, "a table's total count is above 2^53: its fp64 sum depends on the order of addition");
  dq_freq_distance r{};
  r.n = (int64_t)n;
  r.m = (int64_t)m;
  r.groups_a = (int64_t)w[4];
  r.groups_b = (int64_t)w[7];
  if (r.groups_a == 0 || r.groups_b == 0) {  // 0L / 0.0 on the empty side: NaN for every key there is
    r.linf_simple = r.groups_a == 0 && r.groups_b == 0 ? 0.0 : std::numeric_limits<double>::quiet_NaN();
    *out = r;
    return DQ_OK;
  }
  unsigned long long res[2];
  DQ_HIP(launch_freq_linf(a->view(), b->view(), (double)r.n, (double)r.m, d, d + 1, a->stream));
  DQ_HIP(hipMemcpyAsync(res, d, sizeof(res), hipMemcpyDeviceToHost, a->stream));
  DQ_HIP(hipStreamSynchronize(a->stream));
  r.groups_common = (int64_t)res[1];
  if (r.groups_common < r.groups_b) {  // keys only in b
    DQ_HIP(launch_freq_linf(b->view(), a->view(), (double)r.m, (double)r.n, d, nullptr, a->stream));
    DQ_HIP(hipMemcpyAsync(res, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, a->stream));
    DQ_HIP(hipStreamSynchronize(a->stream));
  }
  std::memcpy(&r.linf_simple, &res[0], sizeof(double));
  if (r.n == 0 || r.m == 0) r.linf_simple = std::numeric_limits<double>::quiet_NaN();  // (groups of count 0 only)
  *out = r;
  return DQ_OK;
}

// MutualInformation over one device state of two key columns (MutualInformation.scala:38-81): see
// dq_freq.hip "MutualInformation".  Words of f->d_dist: {f's lo / hi / groups (totals), the first
// marginal's groups (unused) / heap use / overflow, the second's, the sum's low / high word, its
// flags, the first marginal's lo / hi / groups (totals), the second's}.
// The marginal tables are scratch: sized for f's groups and heap use (no growth, no retry) and
// released on return.
extern "C" dq_status dq_freq_mutual_information(dq_freq* f, dq_freq_mi* out) {
  if (!f) return fail(DQ_ERR_INVALID, "NULL table");
  if (!out) return fail(DQ_ERR_INVALID, "NULL argument");
  if (f->ks.n_keys != 2) return fail(DQ_ERR_INVALID, "MutualInformation needs a table that groups exactly two key columns");
  if (f->ks.null_as_key) return fail(DQ_ERR_INVALID, "MutualInformation is not defined over a Histogram (NULL-as-key) table");
  const int type_a = f->col_types[f->ks.key_cols[0]], type_b = f->col_types[f->ks.key_cols[1]];
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize());
  unsigned long long h[FC_COUNT];
  DQ_TRY(f->read_counters(h));
  dq_freq_mi r{};
  r.mi = std::numeric_limits<double>::quiet_NaN();
  r.num_rows = f->num_rows;
  if (h[FC_GROUPS] == 0) {  // (the analyzer reports the empty state)
    *out = r;
    return DQ_OK;
  }
  if (f->num_rows < 0 || f->num_rows > ((int64_t)1 << 53))
    return fail(DQ_ERR_UNSUPPORTED, "the table's numRows is above 2^53: not exact as the fp64 total of the reference");
  constexpr int kWords = 18;
  DQ_TRY(f->d_dist.ensure(kWords * sizeof(unsigned long long)));
  unsigned long long* d = static_cast<unsigned long long*>(f->d_dist.ptr);
  unsigned long long w[kWords] = {};
  DQ_HIP(hipMemsetAsync(d, 0, sizeof(w), f->stream));
  DQ_HIP(launch_freq_totals(f->view(), d, f->stream));
  DQ_HIP(hipMemcpyAsync(w, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  const unsigned __int128 n = ((unsigned __int128)w[1] << 32) + w[0];
  r.groups = (int64_t)w[2];
  if (r.groups == 0) {
    *out = r;
    return DQ_OK;
  }
  if (n > (unsigned __int128)f->num_rows)
    return fail(DQ_ERR_UNSUPPORTED, "the table's counts sum to more than its numRows: a probability above 1 has no bounded term");
  uint64_t cap = kFreqSliceSlots;
  while (cap < 2 * (uint64_t)r.groups) cap <<= 1;
  DevBuf slots[2], heap[2];
  FreqTable T[2];
  for (int i = 0; i < 2; ++i) {
    DQ_TRY(slots[i].ensure(cap * sizeof(FreqSlot)));
    DQ_TRY(heap[i].ensure((size_t)h[FC_HEAP_USED] + 8));
    DQ_HIP(hipMemsetAsync(slots[i].ptr, 0, cap * sizeof(FreqSlot), f->stream));
    T[i].slots = static_cast<FreqSlot*>(slots[i].ptr);
    T[i].mask = cap - 1;
    T[i].bucket_bits = slice_bits_for(cap);
    T[i].test_flags = 0;
    T[i].n_groups = d + 3 + 3 * i;
    T[i].heap = static_cast<uint8_t*>(heap[i].ptr);
    T[i].heap_used = d + 4 + 3 * i;
    T[i].heap_cap = heap[i].cap;
    T[i].overflow = reinterpret_cast<unsigned int*>(d + 5 + 3 * i);
  }
  const FreqTable X = f->view();
  DQ_HIP(launch_freq_mi_project(X, T[0], T[1], type_a, type_b, reinterpret_cast<unsigned int*>(d + 11), f->stream));
  DQ_HIP(launch_freq_mi_sum(X, T[0], T[1], type_a, type_b, (double)f->num_rows, d + 9, f->stream));
  DQ_HIP(launch_freq_totals(T[0], d + 12, f->stream));
  DQ_HIP(launch_freq_totals(T[1], d + 15, f->stream));
  DQ_HIP(hipMemcpyAsync(w, d, sizeof(w), hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));  // (the scratch tables are released below: the stream is idle)
  const unsigned int flags = (unsigned int)w[11];
  if (flags & kMiBadKey) return fail(DQ_ERR_INVALID, "a group key does not split into the table's two key columns");
  if ((flags & kMiNoGroup) || (unsigned int)w[5] || (unsigned int)w[8])
    return fail(DQ_ERR_DEVICE, "MutualInformation: a marginal group could not be placed or found (internal)");
  for (int i = 0; i < 2; ++i)  // every joint count went to exactly one group of either marginal
    if ((((unsigned __int128)w[13 + 3 * i] << 32) + w[12 + 3 * i]) != n)
      return fail(DQ_ERR_DEVICE, "MutualInformation: a marginal table's counts do not sum to the joint table's (internal)");
  r.groups_a = (int64_t)w[14];
  r.groups_b = (int64_t)w[17];
  if (!(flags & kMiNanTerm)) {
    const mi::u128 sum = ((mi::u128)w[10] << 64) | (mi::u128)w[9];
    r.mi = mi::from_fixed((mi::i128)sum);
  }
  *out = r;
  return DQ_OK;
}

// ---------------------------------------------------------------- multi-GPU key-hash exchange
extern "C" dq_status dq_freq_partition(dq_freq* f, int n_parts, void* d_out, int64_t out_bytes, uint8_t* d_key_bytes,
                                       int64_t key_cap, int64_t* part_packed, int64_t* part_groups,
                                       int64_t* part_key_bytes) {
  if (!f || !part_packed || !part_groups || !part_key_bytes) return fail(DQ_ERR_INVALID, "NULL argument");
  if (n_parts < 1 || n_parts > 4096) return fail(DQ_ERR_INVALID, "n_parts out of range [1, 4096]");
  DQ_HIP(hipSetDevice(f->ctx->device));
  DQ_TRY(f->materialize());
  // counters per (part, kind, chunk of slices), chunks as fine as 2^22 counters allow
  const uint64_t n_slices = f->capacity >> kFreqSliceLog;
  int chunk_log = 0;
  while ((n_slices >> chunk_log) > 1 && (n_slices >> chunk_log) * 2ull * (uint64_t)n_parts > (1ull << 22)) ++chunk_log;
  const uint64_t n_chunks = std::max<uint64_t>(1, n_slices >> chunk_log);
  const uint64_t n_cnt = 2ull * (uint64_t)n_parts * n_chunks;
  const size_t words = (size_t)(n_cnt + 1) + (size_t)(n_cnt / 4096 + 2) + (size_t)(2 * n_parts + 1) + 7 * (size_t)n_parts;
  DQ_TRY(f->d_part.ensure(words * sizeof(unsigned long long)));
  unsigned long long* cnt = static_cast<unsigned long long*>(f->d_part.ptr);
  unsigned long long* sums = cnt + (n_cnt + 1);
  unsigned long long* gath = sums + (n_cnt / 4096 + 2);
  unsigned long long* kbytes = gath + (2 * n_parts + 1);
  unsigned long long* sec = kbytes + n_parts;       // 4 per part
  unsigned long long* key_base = sec + 4 * n_parts;
  unsigned long long* key_cur = key_base + n_parts;
  DQ_HIP(hipMemsetAsync(cnt + n_cnt, 0, sizeof(unsigned long long), f->stream));
  DQ_HIP(hipMemsetAsync(kbytes, 0, (size_t)n_parts * sizeof(unsigned long long), f->stream));
  DQ_HIP(launch_wire_count(f->view(), n_parts, chunk_log, n_chunks, cnt, kbytes, f->stream));
  DQ_HIP(scan_exclusive_u64(cnt, n_cnt + 1, sums, f->stream));
  DQ_HIP(launch_gather_strided(cnt, n_chunks, 2ull * (uint64_t)n_parts, gath, f->stream));
  std::vector<unsigned long long> g(2 * n_parts + 1), kb(n_parts);
  DQ_HIP(hipMemcpyAsync(g.data(), gath, g.size() * 8, hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipMemcpyAsync(kb.data(), kbytes, kb.size() * 8, hipMemcpyDeviceToHost, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  int64_t total_b = 0, total_k = 0;
  std::vector<unsigned long long> hsec(4 * (size_t)n_parts), hkb(n_parts);
  for (int p = 0; p < n_parts; ++p) {
    part_packed[p] = (int64_t)(g[2 * p + 1] - g[2 * p]);
    part_groups[p] = (int64_t)(g[2 * p + 2] - g[2 * p + 1]);
    part_key_bytes[p] = (int64_t)kb[p];
    hsec[4 * p] = (unsigned long long)total_b;
    hsec[4 * p + 1] = g[2 * p];
    hsec[4 * p + 2] = g[2 * p + 1];
    hsec[4 * p + 3] = (unsigned long long)part_packed[p];
    hkb[p] = (unsigned long long)total_k;
    total_b += 16 * part_packed[p] + 32 * part_groups[p];
    total_k += part_key_bytes[p];
  }
  if (total_b > out_bytes || total_k > key_cap || (total_b > 0 && !d_out) || (total_k > 0 && !d_key_bytes))
    return fail(DQ_ERR_SPACE, "partition buffers too small (sizes returned)");
  if (total_b == 0) return DQ_OK;
  DQ_HIP(hipMemcpyAsync(sec, hsec.data(), hsec.size() * 8, hipMemcpyHostToDevice, f->stream));
  DQ_HIP(hipMemcpyAsync(key_base, hkb.data(), hkb.size() * 8, hipMemcpyHostToDevice, f->stream));
  DQ_HIP(hipMemsetAsync(key_cur, 0, (size_t)n_parts * sizeof(unsigned long long), f->stream));
  DQ_HIP(launch_wire_scatter(f->view(), n_parts, chunk_log, n_chunks, cnt, sec, key_base, key_cur,
                             static_cast<uint8_t*>(d_out), d_key_bytes, f->stream));
  DQ_HIP(hipStreamSynchronize(f->stream));
  return DQ_OK;
}

extern "C" dq_status dq_freq_import_parts(dq_freq* f, int n_parts, const void* d_parts, const int64_t* part_packed,
                                          const int64_t* part_groups, const uint8_t* d_key_bytes,
                                          const int64_t* part_key_bytes, int64_t num_rows) {
  if (!f || n_parts < 0 || (n_parts > 0 && (!part_packed || !part_groups || !part_key_bytes)))
    return fail(DQ_ERR_INVALID, "bad argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  std::vector<ImportRun> runs;
  const uint8_t* base = static_cast<const uint8_t*>(d_parts);
  uint64_t off = 0, koff = 0, heap = 0;
  for (int p = 0; p < n_parts; ++p) {
    if (part_packed[p] < 0 || part_groups[p] < 0 || part_key_bytes[p] < 0) return fail(DQ_ERR_INVALID, "negative part size");
    if ((part_packed[p] || part_groups[p]) && !d_parts) return fail(DQ_ERR_INVALID, "NULL parts");
    if (part_packed[p]) runs.push_back(ImportRun{base + off, (uint64_t)part_packed[p], nullptr, 0, 0, 0, 0});
    off += 16ull * (uint64_t)part_packed[p];
    if (part_groups[p]) runs.push_back(ImportRun{base + off, (uint64_t)part_groups[p], d_key_bytes + koff, 1, 0, 0, 0});
    off += 32ull * (uint64_t)part_groups[p];
    koff += (uint64_t)part_key_bytes[p];
    heap += (uint64_t)part_key_bytes[p];
  }
  DQ_TRY(f->materialize_for_write());
  f->num_rows += num_rows;
  return f->import_runs(runs, -1, heap);
}

extern "C" dq_status dq_freq_import_wire(dq_freq* f, const dq_freq_wire* d_groups, int64_t n,
                                         const uint8_t* d_key_bytes, int64_t key_bytes, int64_t num_rows) {
  if (!f || (n > 0 && !d_groups) || n < 0 || key_bytes < 0) return fail(DQ_ERR_INVALID, "bad argument");
  const int64_t zero = 0;
  return dq_freq_import_parts(f, 1, d_groups, &zero, &n, d_key_bytes, &key_bytes, num_rows);
}

extern "C" dq_status dq_freq_count_histogram(dq_freq* f, int64_t* hist, int64_t n_bins, int64_t* big,
                                             int64_t big_cap, int64_t* n_big) {
  if (!f || !hist || !n_big || n_bins < 2 || (big_cap > 0 && !big)) return fail(DQ_ERR_INVALID, "bad argument");
  DQ_HIP(hipSetDevice(f->ctx->device));
  std::vector<unsigned long long> h, b;
  DQ_TRY(freq_hist(f, h, b));
  std::memset(hist, 0, (size_t)n_bins * sizeof(int64_t));
  std::vector<int64_t> over;
  for (int c = 1; c < kFreqHist; ++c) {
    if (!h[c]) continue;
    if (c < n_bins) hist[c] = (int64_t)h[c];
    else over.insert(over.end(), (size_t)h[c], (int64_t)c);
  }
  for (unsigned long long c : b) {
    if ((int64_t)c < n_bins) hist[c] += 1;
    else over.push_back((int64_t)c);
  }
  std::sort(over.begin(), over.end());
  *n_big = (int64_t)over.size();
  if ((int64_t)over.size() > big_cap) return fail(DQ_ERR_SPACE, "big-count buffer too small (size returned)");
  if (!over.empty()) std::memcpy(big, over.data(), over.size() * sizeof(int64_t));
  return DQ_OK;
}

extern "C" dq_status dq_freq_summary_from_histogram(const int64_t* hist, int64_t n_bins, const int64_t* big,
                                                    int64_t n_big, int64_t num_rows, dq_freq_summary* out) {
  if (!hist || !out || n_bins < 2 || n_big < 0 || (n_big > 0 && !big)) return fail(DQ_ERR_INVALID, "bad argument");
  std::vector<unsigned long long> h((size_t)n_bins), b((size_t)n_big);
  for (int64_t c = 0; c < n_bins; ++c) h[c] = (unsigned long long)hist[c];
  for (int64_t i = 0; i < n_big; ++i) b[i] = (unsigned long long)big[i];
  std::sort(b.begin(), b.end());
  summary_from_hist(h, b, num_rows, out);
  return DQ_OK;
}
