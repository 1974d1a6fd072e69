/*
 * deequ_amd_diag.h -- measurement entry points of libdeequ_amd.so.  Not part of the drop-in
 * boundary (deequ_amd.h): no reference call site binds these.  bench.py uses them to price
 * the hash-bound kernels (ApproxCountDistinct, StatefulHyperloglogPlus.scala:89-115) against
 * the VALU hash rate the card sustains, next to the HBM roofline.
 */
#ifndef DEEQU_AMD_DIAG_H
#define DEEQU_AMD_DIAG_H

#include <stdint.h>
#include "deequ_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Runs `reps` launches of a register-only kernel that hashes int64 values with Spark's
 * XXH64 (seed 42), and with `with_hll` != 0 also takes each hash's HLL index/rank and folds it
 * into an LDS register copy, on `device`; no HBM traffic.  Writes the sustained hash rate
 * (hashes per second, best launch) to *hashes_per_sec. */
dq_status dq_diag_hash_rate(int device, int with_hll, int reps, double* hashes_per_sec);

/* Aggregates what `f` has staged, then reports which paths its groupings took (tests assert
 * that a workload exercised the path it is meant to): out[0] = table slots (2048 per slice),
 * out[1] = partition-path aggregations, out[2] = hash bits (log2 slices) of the last one,
 * out[3] = records that went through the sort path (small stagings, retries, skew fallbacks),
 * out[4] = partition-path aggregations of packed digit-key records, out[5] = batches grouped by
 * the few-groups kernel (dq_freq_small_kernel), out[6] = 1 if a wait for another lane's slot
 * publish ever timed out (an error every API call also reports), out[7] = imported wire runs
 * that were in order only by coarser slices than the table's (merged from the enclosing ranges),
 * out[8] = imported wire runs out of order (inserted group by group), out[9] = partition-path
 * aggregations of hashed records (long or multi-column keys), out[10] = hashed records inserted
 * globally (slices handed back, tables that already held groups), out[11] = 1 while the table is
 * compacted (occupied slots only), out[12] = partition-path aggregations of canonical UUID records
 * (dq_uuidpack.h), out[13] = partition-path aggregations of 16-byte-key records (16-byte strings,
 * two 8-byte key columns), out[14] = batches rolled back out of the staging regions (staged again in
 * another record format or grouped on the general path), out[15] = times the staged regions were
 * aggregated because a batch of another record format arrived, out[16] = the key heap's cursor in
 * bytes (what a rolled-back hashed staging puts back).  `out` holds 17 values. */
dq_status dq_diag_freq_paths(dq_freq* f, int64_t* out);

/* Test hooks of one table (tests only; never set by the product): flags = 1 makes claimed
 * global slots never turn READY, so a wait for another lane's publish times out (the timeout is
 * a hard error, DQ_ERR_DEVICE).  0 restores normal publishing.  Replaces an environment variable
 * the production library used to read on every dq_freq_create. */
dq_status dq_diag_freq_test_flags(dq_freq* f, int32_t flags);

/* Host build of the library's java.lang.Double.parseDouble (the parser dq_cast_utf8 and the
 * predicate IR's string -> double cast run on the device, compiled from the same source):
 * *ok = 1 and *out = the correctly rounded value, or *ok = 0 (NumberFormatException, NULL in
 * Spark).  Lets CPU tests check it against a reference parser on millions of strings. */
dq_status dq_diag_parse_double(const uint8_t* s, int64_t n, double* out, int32_t* ok);

/* Host build of the predicate interpreter (the source dq_pred_kernel runs on the device,
 * deequ_amd/csrc/dq_predeval.h): validates `p` against the columns' types as plan creation does
 * (same status codes), then evaluates it over `n_rows` rows of HOST columns (offset 0):
 * out[r] = 0 FALSE, 1 TRUE, 2 NULL.  CPU tests check it against the oracle's SQL evaluator. */
dq_status dq_diag_eval_predicate(const dq_predicate* p, const dq_column* columns, int n_columns, int64_t n_rows,
                                 uint8_t* out);

/* Host build of the cross-table checks' NULL-safe cell equality (the source dq_freq_match_rows runs
 * on the device, deequ_amd/csrc/dq_celleq.h): *equal = row i of `a` <=> row j of `b`, two HOST
 * columns of one type, read at their `offset`.  DQ_ERR_INVALID for two types or a row outside a
 * column. */
dq_status dq_diag_cell_equal(const dq_column* a, int64_t i, const dq_column* b, int64_t j, int32_t* equal);

/* Host build of the group-by's record packing of digit-string keys (<= 15 ASCII digits, or
 * Histogram's "NullValue"; deequ_amd/csrc/dq_keypack.h): *ok = 1, *packed = the 8-byte record
 * word and back[0 .. *back_len) = the key bytes it unpacks to; *ok = 0 for any other key. */
/* The group-by's table hash of n inline keys (k0/k1 = key bytes little-endian, len <= 16) as the
 * device computes it: out[2i] = the hash, out[2i+1] = the packed record word or ~0 (tests check
 * both against a host restatement). */
dq_status dq_diag_table_hash(int device, const uint64_t* k0, const uint64_t* k1, const uint32_t* len, int64_t n,
                             uint64_t* out);

dq_status dq_diag_key_pack(const uint8_t* key, int32_t len, uint64_t* packed, uint8_t* back, int32_t* back_len,
                           int32_t* ok);

/* Host build of the group-by's canonical-UUID packing (dq_uuidpack.h): *ok = 1 and words[0..1] =
 * the key's 128-bit value, back[0..36) = the text it unpacks to, when key[0..len) is a canonical
 * lowercase UUID ("xxxxxxxx-xxxx-xxxx-xxxx-xxxxxxxxxxxx"); else *ok = 0. */
dq_status dq_diag_uuid_pack(const uint8_t* key, int32_t len, uint64_t* words, uint8_t* back, int32_t* ok);

/* Host build of PatternMatch's regex engine (deequ_amd/csrc/dq_regex.h: the compiler, and the
 * table walker dq_regex_kernel runs on the device): compiles pattern[0 .. pattern_len) as plan
 * creation does (DQ_ERR_UNSUPPORTED with the construct and its offset in dq_last_error for a
 * pattern outside the exact subset), then *matched = 1 when java.util.regex's Matcher.find() would
 * succeed on text[0 .. n) with a non-empty group 0, else 0.  *n_states / *n_classes = the search
 * DFA's table shape (the columns include the end-of-input one).  text may be NULL with n = 0.
 * Each thread keeps the outcome of its last pattern: calls that repeat it do not compile again. */
dq_status dq_diag_regex_match(const uint8_t* pattern, int32_t pattern_len, const uint8_t* text, int64_t n,
                              int32_t* matched, int32_t* n_states, int32_t* n_classes);

/* dq_diag_regex_match in one of the compiler's three matching modes: 0 find with a non-empty group
 * 0 (what dq_diag_regex_match is), 1 find (RLIKE: an empty match counts), 2 full (pattern is a SQL
 * LIKE pattern and the whole text must match).  image (may be NULL) receives the compiled DFA image
 * when image_capacity holds it; *image_len (may be NULL) = its size either way. */
dq_status dq_diag_regex_match_mode(const uint8_t* pattern, int32_t pattern_len, int32_t mode, const uint8_t* text,
                                   int64_t n, int32_t* matched, int32_t* n_states, int32_t* n_classes,
                                   uint8_t* image, int64_t image_capacity, int64_t* image_len);

/* LIKE / RLIKE match tasks of a plan (distinct (column, pattern, mode) over all its predicates and
 * filters) and the distinct DFA images they use.  Host bookkeeping only. */
dq_status dq_diag_plan_match_tasks(dq_plan* plan, int32_t* n_tasks, int32_t* n_images);

/* Host build of KLLSketch's whole layout (deequ_amd/csrc/dq_kll.cpp: the reference's sequential
 * sketch; no GPU): values[r] is row r, NULL where valid[r] == 0 (valid may be NULL: no NULLs); the
 * rows are cut into slabs of slab_rows, each sketched as one reference partition, and the slabs merged
 * by the balanced tree dq_kll_consume uses.  The sketch is written as dq_kll_export writes it
 * (same DQ_ERR_SPACE protocol).  slab_rows >= n gives the plain sequential sketch. */
dq_status dq_diag_kll_sketch(const double* values, const uint8_t* valid, int64_t n, int32_t sketch_size,
                             double shrinking_factor, int64_t slab_rows, void* out, int64_t capacity,
                             int64_t* required);

/* Host build of RowLevelSchemaValidator's int and decimal cell tests (deequ_amd/csrc/dq_schema.h,
 * the source dq_schema_eval_kernel runs on the device) on the non-NULL cell text[0 .. n).
 * kind = DQ_SCHEMA_INT: UTF8String.toInt; kind = DQ_SCHEMA_DECIMAL: new java.math.BigDecimal(text)
 * .setScale(scale, ROUND_HALF_UP) within `precision` (1..18) digits.  *result = 0 the cast is NULL
 * (the cell is invalid), 1 it succeeds and *value = the int / the unscaled decimal, 2 (decimal
 * only) the GPU declines the cell: a byte >= 0x80 or an exponent beyond +-1000. */
dq_status dq_diag_schema_cell(int32_t kind, const uint8_t* text, int64_t n, int32_t precision, int32_t scale,
                              int32_t* result, int64_t* value);

/* Host build of the decimal -> double cast (deequ_amd/csrc/dq_decimal.h, the source the decimal
 * scan and dq_cast_decimal run on the device): the unscaled value lo | hi << 64 (two's complement)
 * at `scale` (0..38), as java.math.BigDecimal.doubleValue rounds it.  *tier = which path took it:
 * 1 one fp64 divide, 2 Eisel-Lemire, 3 the exact long division. */
dq_status dq_diag_decimal_to_double(uint64_t lo, int64_t hi, int32_t scale, double* out, int32_t* tier);

/* Host build of the bytes the decimal scan hashes for a precision > 18 column
 * (java.math.BigInteger.toByteArray of the unscaled value): out[0 .. *len), *len in 1..16. */
dq_status dq_diag_decimal_bytes(uint64_t lo, int64_t hi, uint8_t* out, int32_t* len);

/* Host build of MutualInformation's shared source (deequ_amd/csrc/dq_mi.h, the code the kernels
 * behind dq_freq_mutual_information run on the device).
 * dq_diag_mi_split: the joint key key[0 .. len) of two key columns of types type_a / type_b (DQ_T_*)
 * -> out[0..3] = {offset, length of the first field, offset, length of the second}: a fixed-width
 * field is its bytes, a string field its UTF-8 bytes without the u32 length prefix.  A key that
 * does not split exactly (a length running past the key, a truncated fixed field, bytes left
 * over, a type that is no key type) is DQ_ERR_INVALID; no byte at or past `len` is read.
 * dq_diag_mi_to_fixed: a term as the signed 128-bit integer round-half-even(|term| 2^96) with the
 * term's sign (*lo, *hi = its two's-complement words); NaN, infinities and |term| >= 2^6 are
 * DQ_ERR_INVALID.  dq_diag_mi_from_fixed: the nearest double (ties to even) of that integer / 2^96. */
dq_status dq_diag_mi_split(const uint8_t* key, int64_t len, int32_t type_a, int32_t type_b, int32_t* out);
dq_status dq_diag_mi_to_fixed(double term, uint64_t* lo, int64_t* hi);
dq_status dq_diag_mi_from_fixed(uint64_t lo, int64_t hi, double* out);

/* The grids dq_plan_consume gave the plan's last non-empty batch (host bookkeeping: no kernel, no
 * device read), so that tests can assert which kernel specialisations a plan ran and how many
 * rows each block walked.  *n_groups = the plan's scan groups (one launch each); for the first
 * min(*n_groups, capacity) of them groups[6g + 0..5] = kind (0 dq_scan_bits_kernel, 1
 * dq_scan_values_kernel, 2 dq_scan_fast_kernel), value type (DQ_T_*; 0 for kind 0), np (kind 1:
 * the inline-predicate count 0..4 or 8, -1 = the EXT kernel; kind 2: the fast variant, predicate
 * kind | 8 statistics | 16 HLL), tasks in the group, blocks per task, resident workgroups per CU
 * the occupancy query gave (0 = not asked).  launches[0..6] = blocks per task of the regex, string
 * pass, HLL, DataType, MinLength/MaxLength, Correlation and decimal launches (0 = not launched),
 * launches[7] = the batch's rows, launches[8] = the decimal scan's resident workgroups per CU (0 =
 * not asked), launches[9] = the device's compute units.  `launches` holds 10 values.  Before the
 * first batch every blocks-per-task value is 0. */
dq_status dq_diag_plan_groups(dq_plan* plan, int64_t* groups, int32_t capacity, int32_t* n_groups,
                              int64_t* launches);

/* Which scan tasks of the plan's last non-empty batch ran the lane-mask loop of dq_scan_fast_kernel
 * (host bookkeeping, by the rule the kernel's blocks apply: the launch's variant takes the loop
 * under DQ_SCAN_LANEMASK, and the task's column has no validity bitmap or a 4-byte aligned one).
 * *n_tasks = the plan's scan tasks, in the order dq_diag_plan_groups' groups list them by index;
 * for the first min(*n_tasks, capacity) of them tasks[t] = 1 or 0 (0 for a task of another kernel,
 * and before the first batch). */
dq_status dq_diag_plan_lanemask(dq_plan* plan, int32_t* tasks, int32_t capacity, int32_t* n_tasks);

/* The tiling constants of take (deequ_amd/csrc/dq_take.h), from which tests derive their shapes:
 * out[0] = output rows per workgroup, out[1] = entries per tile of the offsets' scan, out[2] = the
 * cell length from which a wave, not a lane, copies a utf8 cell, out[3] = the length from which a
 * cell is cut into pieces of that size for workgroups of their own.  `out` holds 4 values. */
dq_status dq_diag_take_constants(int64_t* out);

/* Host mirror of one dq_corrmat_consume batch (deequ_amd/csrc/dq_corrmat.h; no GPU): the same
 * slabs, per-column shifts, guard, fall-back flags and merge order, the sums as plain fp64 loops.
 * columns[i][r] = row r of selected column i, already cast to double; valid[i][r] = 0 where it is NULL
 * (valid or valid[i] may be NULL: no NULLs); where[r] = 0 where the filter is not TRUE (NULL: no
 * filter); max_ranges = the row ranges the slabs are spread over (the kernel's grid; < 1: one per
 * slab).  states: 6 doubles per pair as dq_corrmat_finish writes them; flags[p] = 1 where pair p is
 * not answered from the matrix sums (its state then comes from per-slab sums about the slab's means). */
dq_status dq_diag_corrmat_host(const double* const* columns, const uint8_t* const* valid, const uint8_t* where,
                               int32_t n_selected, int64_t n_rows, int64_t max_ranges, double* states, uint8_t* flags);

#ifdef __cplusplus
}
#endif

#endif /* DEEQU_AMD_DIAG_H */
