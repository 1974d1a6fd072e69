/*
 * deequ_amd.h -- C-ABI of the MI355X-native backend for deequ's metric hot path.
 *
 * This is the drop-in boundary named by SURVEY.md §8(b).  In the reference there is no
 * FFI: the seam is the Scala trait pair
 *     ScanShareableAnalyzer.aggregationFunctions() / fromAggregationResult()
 *         (src/main/scala/com/amazon/deequ/analyzers/Analyzer.scala:169-197)
 *     State.sum                                    (Analyzer.scala:34-48)
 * and the single launch site of the fused scan
 *     data.agg(aggs.head, aggs.tail: _*).collect().head   (runners/AnalysisRunner.scala:313)
 * plus the grouping launch site
 *     FrequencyBasedAnalyzer.computeFrequencies   (analyzers/GroupingAnalyzers.scala:53-80).
 * A JNI shim replaces those call sites for GPU-eligible analyzers: it
 * creates a plan from the analyzers, feeds Arrow-layout column batches, and turns the POD
 * states returned here into the unchanged Scala `State` case classes, which then flow into
 * Analyzer.calculateMetric (Analyzer.scala:107-128) exactly as Spark-produced states do.
 *
 * Conventions
 *   - Every function returns dq_status (0 = OK).  No C++ exception crosses the ABI.
 *     dq_last_error() returns a thread-local message for the last failure.
 *   - Columns use the Arrow layout: validity bitmap LSB-first, 1 = valid (NULL pointer = no
 *     nulls), fixed-width values, utf8 = int32 offsets + bytes.  A column's buffers are either
 *     host memory (copied to HBM by the library) or device memory on the context's GPU
 *     (DQ_COL_DEVICE; used in place, never copied).  Only rows [offset, offset + length) and
 *     their validity bits are a column's content: what NULL slots hold (values, or the heap
 *     bytes a NULL string spans), the bitmap's padding bits, and the rows, bits and heap bytes
 *     outside the window are ignored (pinned by tests/test_gpu_hostile_*.py).
 *   - Plans are not thread-safe; use one plan per calling thread.  Contexts may be shared.
 */
#ifndef DEEQU_AMD_H
#define DEEQU_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_ABI_VERSION 4

/* ---------------------------------------------------------------- status codes */
typedef enum dq_status {
  DQ_OK = 0,
  DQ_ERR_INVALID = 1,      /* bad argument (maps to IllegalArgumentException)           */
  DQ_ERR_UNSUPPORTED = 2,  /* op/type/predicate not on the GPU path: route it to Spark   */
  DQ_ERR_DEVICE = 3,       /* HIP runtime failure or no usable gfx950 device             */
  DQ_ERR_OOM = 4,          /* device allocation failed                                   */
  DQ_ERR_STATE = 5,        /* call out of order (e.g. consume after finish without reset)*/
  DQ_ERR_SPACE = 6         /* caller's output buffer too small: required sizes returned  */
} dq_status;

/* ---------------------------------------------------------------- column types */
typedef enum dq_type {
  DQ_T_BOOL = 1,     /* Arrow bit-packed boolean                    (Spark BooleanType) */
  DQ_T_INT8 = 2,     /*                                             (ByteType)          */
  DQ_T_INT16 = 3,    /*                                             (ShortType)         */
  DQ_T_INT32 = 4,    /*                                             (IntegerType)       */
  DQ_T_INT64 = 5,    /*                                             (LongType)          */
  DQ_T_FLOAT32 = 6,  /*                                             (FloatType)         */
  DQ_T_FLOAT64 = 7,  /*                                             (DoubleType)        */
  DQ_T_UTF8 = 8,     /* int32 offsets + UTF-8 bytes                 (StringType)        */
  DQ_T_DECIMAL128 = 9 /* Arrow decimal128: 16 little-endian bytes per row, the two's-complement
                         unscaled value                              (DecimalType(p, s)) */
} dq_type;

/* A decimal column's type code carries its precision and scale in the same int32 that every
 * *_create / dq_op_supported takes and dq_column.type holds: DQ_T_DECIMAL(p, s) with precision
 * 1..38 and scale 0..p (anything else is DQ_ERR_INVALID).  The low byte is the dq_type.
 * Decimal columns serve Completeness, Sum, Mean, Minimum, Maximum, StandardDeviation and
 * ApproxCountDistinct (one fused pass, dq_scan_dec.hip), `IS [NOT] NULL` in predicates, and
 * dq_cast_decimal; every other op, a decimal grouping column of dq_freq_create, a decimal column
 * sketched by dq_kll_create / dq_aq_create and a decimal column among dq_schema_create's /
 * dq_schema_supported's input columns are DQ_ERR_UNSUPPORTED. */
#define DQ_T_DECIMAL(p, s) ((int32_t)(DQ_T_DECIMAL128 | ((p) << 8) | ((s) << 16)))
#define DQ_T_BASE(t) ((int32_t)((t) & 0xff))
#define DQ_T_PRECISION(t) ((int32_t)(((t) >> 8) & 0xff))
#define DQ_T_SCALE(t) ((int32_t)(((t) >> 16) & 0xff))

#define DQ_COL_DEVICE 0x1 /* validity/values/offsets are device pointers on ctx's GPU */

typedef struct dq_column {
  int32_t type;             /* dq_type; DQ_T_DECIMAL(p, s) for a decimal column          */
  int32_t flags;            /* DQ_COL_*                                                  */
  int64_t length;           /* number of rows in this batch                             */
  int64_t offset;           /* Arrow slot offset of row 0 (elements; bits for bitmaps)  */
  const uint8_t* validity;  /* LSB-first bitmap, 1 = valid; NULL = no nulls             */
  const void* values;       /* fixed-width values (decimal: 16 B each), bit-packed bools, or utf8 bytes */
  const int32_t* offsets;   /* utf8 only: length+1 offsets (from `offset`)              */
} dq_column;

/* ---------------------------------------------------------------- analyzer ops */
typedef enum dq_op_kind {
  DQ_OP_SIZE = 1,                  /* Size(where)                       Size.scala:35-47        */
  DQ_OP_COMPLETENESS = 2,          /* Completeness(column, where)       Completeness.scala:26-46*/
  DQ_OP_COMPLIANCE = 3,            /* Compliance(instance, pred, where) Compliance.scala:37-53  */
  DQ_OP_SUM = 4,                   /* Sum(column, where)                Sum.scala:35-52         */
  DQ_OP_MEAN = 5,                  /* Mean(column, where)               Mean.scala:36-54        */
  DQ_OP_STDDEV = 6,                /* StandardDeviation(column, where)  StandardDeviation.scala:47-73 */
  DQ_OP_MINIMUM = 7,               /* Minimum(column, where)            Minimum.scala:35-53     */
  DQ_OP_MAXIMUM = 8,               /* Maximum(column, where)            Maximum.scala:35-53     */
  DQ_OP_APPROX_COUNT_DISTINCT = 9, /* ApproxCountDistinct(column, where) ApproxCountDistinct.scala:47-64 */
  DQ_OP_DATATYPE = 10,             /* DataType(column, where)           DataType.scala:152-183  */
  DQ_OP_MIN_LENGTH = 11,           /* MinLength(column, where)          MinLength.scala:25-41   */
  DQ_OP_MAX_LENGTH = 12,           /* MaxLength(column, where)          MaxLength.scala:25-41   */
  DQ_OP_CORRELATION = 13,          /* Correlation(column, column2, where) Correlation.scala:77-105 */
  DQ_OP_PATTERN_MATCH = 14         /* PatternMatch(column, pattern, where) PatternMatch.scala:37-55: a
                                      utf8 column; the pattern text (pattern.toString, UTF-8) travels as
                                      predicate.strings[0 .. strings_len) with predicate.n_insns = 0.  A
                                      pattern outside the exact subset (PatternMatch) is
                                      DQ_ERR_UNSUPPORTED at plan time                                   */
} dq_op_kind;

/*
 * Predicate IR: an analyzed Catalyst boolean expression (casts resolved) in postfix form.
 * It covers what deequ's Check DSL emits for numeric columns (Check.scala:594-943:
 * comparisons, COALESCE, IN, BETWEEN, IS [NOT] NULL, AND/OR/NOT) with SQL three-valued
 * logic.  Anything else is rejected with DQ_ERR_UNSUPPORTED at plan time.
 *
 * Value instructions push a typed value (int64, fp64 or UTF-8 string, each with a NULL flag);
 * boolean instructions pop/push three-valued booleans.  Numeric comparisons compare in the type
 * given by `arg` (DQ_CMP_AS_INT64 / DQ_CMP_AS_FLOAT64), converting operands first; two strings
 * compare byte-wise (unsigned, then by length), as Spark's UTF8String.compareTo.
 *
 * Type rules the library enforces (anything it cannot evaluate exactly as Spark would is
 * DQ_ERR_UNSUPPORTED, so the caller routes the analyzer to Spark; a malformed program -- stack
 * underflow, a column out of range -- is DQ_ERR_INVALID):
 *   - DQ_CMP_AS_INT64 with a floating-point operand;
 *   - a FloatType value (a FLOAT32 column or DQ_P_CAST to FLOAT32) compared or COALESCEd with an
 *     integral operand: Spark coerces that pair to FloatType, so the integral side must carry an
 *     explicit DQ_P_CAST to FLOAT32 (an integral literal may instead be rounded to float by the
 *     encoder and pushed with DQ_P_LIT_FLOAT);
 *   - a string compared with a non-string (only DQ_P_CAST_DOUBLE converts strings);
 *   - DQ_P_CAST of a string.
 */
typedef enum dq_pred_opcode {
  DQ_P_COLUMN = 1,     /* push value of batch column `arg`                                  */
  DQ_P_LIT_INT = 2,    /* push int64 literal `i64`                                          */
  DQ_P_LIT_FLOAT = 3,  /* push fp64 literal `f64`                                           */
  DQ_P_LIT_NULL = 4,   /* push NULL                                                         */
  DQ_P_COALESCE = 5,   /* pop b, a; push a if a non-NULL else b                             */
  DQ_P_LIT_STRING = 6, /* push UTF-8 literal strings[i64 .. i64 + arg) of the predicate      */
  DQ_P_CAST_DOUBLE = 7, /* pop value; push it as fp64: Spark 2.2 Cast(-> DoubleType), which a
                           comparison of a string with a number inserts (PromoteStrings): a string
                           through java.lang.Double.parseDouble of its trimmed text, NULL when
                           unparsable; correctly rounded for every input (decimal of any
                           length and exponent, hexadecimal, NaN / Infinity, f/d suffix).   */
  DQ_P_CAST = 8,       /* pop value; push Cast(value -> `arg`), `arg` a dq_type: INT8..INT64,
                           FLOAT32, FLOAT64 or BOOL, of a numeric or boolean value (Spark 2.2.2
                           Cast, non-ANSI: integral narrowing keeps the low bits; fractional ->
                           int/long is Java d2i/d2l, NaN -> 0, saturating; -> short/byte is d2i
                           then the low bits; integral -> float rounds the integer itself (l2f);
                           -> boolean is value != 0; boolean -> numeric 1/0).  The analyzer's
                           Cast nodes (`cast(l as int) > 3`, the FloatType side of `f = 16777217`)
                           map 1:1 onto it.  A cast of a string other than DQ_P_CAST_DOUBLE is
                           DQ_ERR_UNSUPPORTED (route the analyzer to Spark).                     */
  DQ_P_EQ = 10, DQ_P_NE = 11, DQ_P_LT = 12, DQ_P_LE = 13, DQ_P_GT = 14, DQ_P_GE = 15,
  DQ_P_EQ_NULLSAFE = 16, /* <=>                                                             */
  DQ_P_IS_NULL = 20,   /* pop value; push boolean (never NULL)                              */
  DQ_P_IS_NOT_NULL = 21,
  DQ_P_AND = 30, DQ_P_OR = 31, DQ_P_NOT = 32,
  DQ_P_TRUE = 33, DQ_P_FALSE = 34,
  DQ_P_LIKE = 40,      /* pop pattern, value; push boolean: Catalyst's Like(left, right) of the
                           analyzed expression (before LikeSimplification).  `_` is one code point,
                           `%` any sequence of them (line terminators included), every other
                           character itself; the whole value must match; NULL where the value is.
                           Accepted only as the triple DQ_P_COLUMN (a utf8 column), DQ_P_LIT_STRING,
                           DQ_P_LIKE; any other operand shape, a pattern that holds a backslash and
                           a pattern whose DFA is over the construction bounds are
                           DQ_ERR_UNSUPPORTED.                                               */
  DQ_P_RLIKE = 41      /* the same for RLike(left, right) (RLIKE / REGEXP): TRUE when
                           Pattern.compile(regex).matcher(value).find(0) -- any match, an empty one
                           included.  The regex subset and its declines are PatternMatch's
                           (DESIGN.md), without the "can match the empty string" decline.       */
} dq_pred_opcode;

#define DQ_CMP_AS_INT64 0
#define DQ_CMP_AS_FLOAT64 1

typedef struct dq_pred_insn {
  int32_t opcode;  /* dq_pred_opcode                                   */
  int32_t arg;     /* column index (DQ_P_COLUMN) or DQ_CMP_AS_* (cmp)  */
  int64_t i64;
  double f64;
} dq_pred_insn;

typedef struct dq_predicate {
  const dq_pred_insn* code;  /* NULL/0 = no predicate                     */
  int32_t n_insns;
  int32_t strings_len;       /* bytes in `strings`                        */
  const uint8_t* strings;    /* pool for DQ_P_LIT_STRING (may be NULL)    */
} dq_predicate;

typedef struct dq_op {
  int32_t kind;              /* dq_op_kind                                     */
  int32_t column;            /* batch column index; ignored for SIZE/COMPLIANCE */
  int32_t column2;           /* CORRELATION: the second column (secondColumn)    */
  int32_t reserved;          /* 0                                                */
  dq_predicate predicate;    /* COMPLIANCE; PATTERN_MATCH: the pattern text    */
  dq_predicate where;        /* optional filter (Analyzers.conditionalSelection) */
} dq_op;

/* ---------------------------------------------------------------- states */
#define DQ_HLL_NUM_WORDS 52   /* StatefulHyperloglogPlus.scala:154 */

/*
 * POD image of the Scala State returned for one op.  `has_value` = 0 is Scala `None`
 * (Spark returned SQL NULL, e.g. Mean over an all-NULL column).  Which fields are meaningful
 * depends on `kind`:
 *   SIZE                         NumMatches(num_matches)
 *   COMPLETENESS, COMPLIANCE,
 *   PATTERN_MATCH                NumMatchesAndCount(num_matches, count)
 *   SUM                          SumState(sum)
 *   MEAN                         MeanState(sum, count)
 *   STDDEV                       StandardDeviationState(n, avg, m2)
 *   MINIMUM / MAXIMUM            MinState(value) / MaxState(value)
 *   APPROX_COUNT_DISTINCT        ApproxCountDistinctState(words)  (always has_value = 1)
 *   DATATYPE                     DataTypeHistogram(words[0..4] = numNull, numFractional,
 *                                numIntegral, numBoolean, numString)  (always has_value = 1:
 *                                the StatefulDataType UDAF never returns NULL)
 *   MIN_LENGTH / MAX_LENGTH      MinState(value) / MaxState(value) of the string lengths
 *   CORRELATION                  CorrelationState(n, avg = xAvg, y_avg, ck, x_mk, y_mk)
 */
typedef struct dq_state {
  int32_t kind;
  int32_t has_value;
  int64_t num_matches;
  int64_t count;
  double sum;
  double n, avg, m2;
  double value;
  int64_t words[DQ_HLL_NUM_WORDS];
  double y_avg, ck, x_mk, y_mk;  /* CORRELATION (with n, avg) */
} dq_state;

/* ---------------------------------------------------------------- context / plan */
typedef struct dq_ctx dq_ctx;
typedef struct dq_plan dq_plan;

const char* dq_last_error(void);
int dq_abi_version(void);

/* Number of gfx950 devices visible to this process (0 on a host without a GPU). */
dq_status dq_device_count(int* out);

/* Give the device blocks the library keeps cached for reuse (every buffer a plan or frequency
 * table freed -- staging, sort buffers, tables; at most 128 GiB -- kept so that a free is not a
 * device-wide hipFree synchronisation) back to the HIP runtime.  No reference counterpart:
 * Spark's executors free their memory through the JVM. */
dq_status dq_release_cached_memory(int device);

dq_status dq_ctx_create(int device, int flags, dq_ctx** out);
dq_status dq_ctx_destroy(dq_ctx* ctx);

/* Build a plan for `n_ops` analyzers over batches with `n_columns` columns of the given
 * types.  All scan-shareable ops of a plan run in one fused pass per batch
 * (AnalysisRunner.scala:306-313).  Returns DQ_ERR_UNSUPPORTED (and sets *out = NULL) if any
 * op cannot run on the GPU; the caller then routes that op to Spark. */
dq_status dq_plan_create(dq_ctx* ctx, const dq_op* ops, int n_ops,
                         const int32_t* column_types, int n_columns, dq_plan** out);
dq_status dq_plan_destroy(dq_plan* plan);

/* dq_plan_create from the analyzer list serialized as bytes -- what the JVM side builds with a
 * little-endian ByteBuffer (GpuPlanEncoder), so the JNI stub passes one byte[]
 * and the library, not hand-written JNI code, decodes and validates it.  Layout:
 *   u32 magic 0x504F5144 ("DQOP"), u32 version 1, u32 n_ops, then per op
 *   i32 kind, i32 column, i32 column2,
 *   i32 n_pred, i32 pred_strings_len, i32 n_where, i32 where_strings_len,
 *   n_pred x {i32 opcode, i32 arg, i64 i64, f64 f64} (24 B), pred_strings_len bytes,
 *   n_where x {...}, where_strings_len bytes.
 * A truncated or inconsistent blob is DQ_ERR_INVALID (checked before any device work). */
#define DQ_PACKED_MAGIC 0x504F5144u
dq_status dq_plan_create_packed(dq_ctx* ctx, const uint8_t* blob, size_t blob_len, const int32_t* column_types,
                                int n_columns, dq_plan** out);

/* Check whether a single op is GPU-eligible for the given schema without building a plan. */
dq_status dq_op_supported(const dq_op* op, const int32_t* column_types, int n_columns);

/* Enqueue one batch (a row partition).  Asynchronous on the plan's HIP stream; host buffers
 * must stay valid until the next dq_plan_* call on this plan returns.  May be called any
 * number of times; results accumulate in HBM in call order (deterministic). */
dq_status dq_plan_consume(dq_plan* plan, const dq_column* columns, int n_columns,
                          int64_t n_rows);

/* Wait for all consumed batches and write one dq_state per op (in op order). */
dq_status dq_plan_finish(dq_plan* plan, dq_state* out, int n_out);

/* Status of op `op` after dq_plan_finish: DQ_OK, or an error the op alone failed with (the
 * per-analyzer scope of AnalysisRunner.scala:340-353: the JNI layer fails or reroutes that
 * analyzer only).  DQ_ERR_UNSUPPORTED: the data made the op one the GPU does not answer (never an
 * approximation) -- a string -> double cast off the exact path in its predicate, or Sum / Mean of a
 * decimal(p, s) column whose sum of |x| reaches 10^min(38, p + 10): Spark 2.2's decimal sum may
 * overflow there, depending on the row order (SPARK-28067). */
dq_status dq_plan_op_status(dq_plan* plan, int op);

/* ---------------------------------------------------------------- Arrow C Data Interface
 * The JVM side of the seam hands Spark partitions over as Arrow record batches
 * (ArrowUtils / ArrowWriter -> org.apache.arrow.c.Data.exportVectorSchemaRoot), i.e. the
 * standard C Data Interface structs below (layout fixed by the Arrow specification).  These
 * entry points replace the hand-filled dq_column array of dq_plan_consume / dq_freq_consume at
 * the launch sites AnalysisRunner.scala:313 (data.agg) and GroupingAnalyzers.scala:53-80.
 *
 * Accepted input: a struct array ("+s", one child per plan column, in plan column order -- a
 * record batch) or a single top-level array (a one-column batch).  Child formats: "b" bool,
 * "c" int8, "s" int16, "i" int32, "l" int64, "f" float32, "g" float64, "u" utf8.  Offsets of
 * sliced arrays (struct offset + child offset) are honoured; a NULL validity buffer means no
 * NULLs.  Rejected with DQ_ERR_UNSUPPORTED (route the batch to Spark): dictionary-encoded,
 * nested, large_utf8 ("U"), decimal ("d:..."; a decimal128 column is handed over as a dq_column of
 * type DQ_T_DECIMAL(p, s) through dq_plan_consume instead), temporal formats and struct-level NULL rows.  Malformed
 * structs (released, buffer counts, children shorter than the batch) give DQ_ERR_INVALID.
 * The caller keeps ownership: release callbacks are never invoked by the library, and the
 * buffers must stay valid until the next call on the plan / table returns (host buffers) or
 * until the plan's stream has drained (DQ_COL_DEVICE: buffers in HBM on the context's GPU). */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif /* ARROW_C_DATA_INTERFACE */

/* Map an Arrow batch onto dq_columns without touching any GPU (pure host; the JNI layer can
 * call it to derive the plan's column types): types[i] / columns[i] for each of the batch's
 * columns (at most max_columns), *n_columns and *n_rows.  `flags` = DQ_COL_DEVICE when the
 * buffers are device pointers.  DQ_ERR_SPACE (with *n_columns set) when max_columns is short. */
dq_status dq_arrow_columns(const struct ArrowSchema* schema, const struct ArrowArray* array, int flags,
                           int32_t* types, dq_column* columns, int max_columns, int* n_columns,
                           int64_t* n_rows);
/* dq_plan_consume of one Arrow batch (its columns in plan column order). */
dq_status dq_plan_consume_arrow(dq_plan* plan, const struct ArrowSchema* schema,
                                const struct ArrowArray* array, int flags);

/* Page-lock a host buffer the caller will hand over again and again (e.g. the JNI layer's Arrow
 * allocator pool), so its batches cross PCIe by DMA at full rate instead of through the
 * runtime's pageable staging; unregister before freeing it.  Host batches are double-buffered in
 * HBM either way: dq_plan_consume returns once a batch's bytes are on the device, while its scan
 * still runs, so the caller fills the next batch during the scan. */
dq_status dq_host_register(void* ptr, size_t bytes);
dq_status dq_host_unregister(void* ptr);

/* Clear accumulated results so the plan can scan a new dataset. */
dq_status dq_plan_reset(dq_plan* plan);

/* The HIP stream (hipStream_t) the plan launches on, for external timing/sync. */
void* dq_plan_stream(dq_plan* plan);

/* ---------------------------------------------------------------- state algebra (host) */
/* `Analyzers.merge` (Analyzer.scala:367-386) over Option[State]: out = a + b with None
 * handling; `a` and `b` must have the same kind.  Mirrors each State.sum. */
dq_status dq_state_merge(const dq_state* a, const dq_state* b, dq_state* out);

/* `DoubleValuedState.metricValue()` of a state with has_value = 1. */
dq_status dq_state_metric(const dq_state* s, double* out);

/* DeequHyperLogLogPlusPlusUtils.count (StatefulHyperloglogPlus.scala:210-257). */
double dq_hll_count(const int64_t words[DQ_HLL_NUM_WORDS]);
/* DeequHyperLogLogPlusPlusUtils.merge (StatefulHyperloglogPlus.scala:188-208). */
void dq_hll_merge(const int64_t a[DQ_HLL_NUM_WORDS], const int64_t b[DQ_HLL_NUM_WORDS],
                  int64_t out[DQ_HLL_NUM_WORDS]);
/* wordsToBytes / wordsFromBytes (StatefulHyperloglogPlus.scala:170-186): 416 big-endian bytes. */
void dq_hll_words_to_bytes(const int64_t words[DQ_HLL_NUM_WORDS], uint8_t out[416]);
void dq_hll_words_from_bytes(const uint8_t in[416], int64_t words[DQ_HLL_NUM_WORDS]);

/* Spark 2.2.2 XxHash64Function with seed 42 for one value (host reference, used by tests). */
uint64_t dq_xxh64(const void* data, size_t len, uint64_t seed);

/* Spark 2.2.2 Cast(StringType -> LongType | DoubleType) of one utf8 column, as
 * ColumnProfiler.castNumericStringColumns does before pass 2 (ColumnProfiler.scala:346-355,
 * 427-445).  Writes n_rows values and a validity bitmap (LSB-first, NULL = unparsable) into
 * DEVICE buffers on ctx's GPU.  Doubles are java.lang.Double.parseDouble, correctly rounded
 * for every input (Clinger's fast path, Eisel-Lemire over a 128-bit power-of-five table, an
 * exact big-integer comparison near rounding boundaries; hexadecimal literals rounded half-even).
 * *n_unsupported is always set to 0 (kept for ABI stability: nothing is routed back). */
dq_status dq_cast_utf8(dq_ctx* ctx, const dq_column* src, int64_t n_rows, int32_t to_type,
                       void* d_values, uint8_t* d_validity, int64_t* n_unsupported);

/* Spark 2.2.2 Cast(DecimalType(p, s) -> DoubleType) of one decimal column: Decimal.toDouble =
 * java.math.BigDecimal.doubleValue, the correctly rounded (ties to even) value of unscaled / 10^s.
 * Writes n_rows doubles and a validity bitmap (LSB-first, bit 0 = row 0; the source's NULLs) into
 * DEVICE buffers on ctx's GPU (values: 8 n_rows bytes; validity: ceil(n_rows / 8) bytes).
 * StandardDeviation casts each row this way inside the decimal scan; Correlation and ApproxQuantile
 * of a decimal column run their float64 paths over this materialised column. */
dq_status dq_cast_decimal(dq_ctx* ctx, const dq_column* src, int64_t n_rows, double* d_values_f64,
                          uint8_t* d_validity);

/* dq_cast_utf8 of n columns of n_rows rows each in one call (castNumericStringColumns casts every
 * string column pass 1 typed numeric): column i (utf8) -> to_types[i] into d_values[i] /
 * d_validity[i].  The casts overlap on the device; the call returns when all are done. */
dq_status dq_cast_utf8_batch(dq_ctx* ctx, int32_t n, const dq_column* srcs, int64_t n_rows,
                             const int32_t* to_types, void* const* d_values, uint8_t* const* d_validity);

/* ApproxCountDistinct and DataType of a utf8 column from its groups instead of its rows: the
 * column's distinct non-NULL strings (flat, as dq_freq_export_flat lists them: counts[i], key
 * bytes [key_offsets[i], key_offsets[i + 1])) and its NULL count.  Every group is hashed and
 * classified once and weighted by its count -- the same registers (a maximum does not see
 * duplicates) and the same five DataType counts as the per-row pass (StatefulHyperloglogPlus
 * .update, StatefulDataType.update over every row).  hll_out / dtype_out receive what
 * dq_plan_finish gives ApproxCountDistinct and DataType on that column.  DQ_FLAT_DEVICE: the
 * three buffers are device memory on the context's device. */
dq_status dq_profile_string_groups(dq_ctx* ctx, const int64_t* counts, const int64_t* key_offsets,
                                   const uint8_t* key_bytes, int64_t n_groups, int64_t n_nulls, int flags,
                                   dq_state* hll_out, dq_state* dtype_out);

/* ColumnProfiler pass 1 on n utf8 columns of one batch, each tried as a few-valued column: the
 * few-groups kernel (per-workgroup LDS tables of DQ_FEW_MAX_GROUPS keys of at most 15 bytes) and
 * one merge per column, all columns in one call (their launches overlap; one wait).  Column i
 * fits when it has at most DQ_FEW_MAX_GROUPS distinct non-NULL strings, none longer than 15
 * bytes (and a string heap of at least 16 bytes); then results[i].ok = 1 and:
 *   - results[i].completeness / .hll / .dtype are what dq_plan_finish gives Completeness,
 *     ApproxCountDistinct and DataType on the column (states from the groups weighted by their
 *     counts: the same registers and counts as the per-row pass);
 *   - its groups are group_counts / group_keys (16 bytes each, zero padded) / group_lens
 *     [i * DQ_FEW_MAX_GROUPS, + results[i].n_groups), non-NULL strings only (NULLs are
 *     results[i].n_nulls).
 * A column that does not fit has ok = 0 and nothing else set.  Columns are grouped 32 at a time
 * (bounded scratch); a chunk whose device scratch cannot be allocated leaves its columns at ok = 0
 * (the caller's per-row pass handles them) instead of failing the call. */
#define DQ_FEW_MAX_GROUPS 1024
typedef struct dq_few_result {
  int32_t ok;
  int32_t n_groups;
  int64_t n_nulls;
  dq_state completeness, hll, dtype;
} dq_few_result;
dq_status dq_profile_few_strings(dq_ctx* ctx, int32_t n, const dq_column* cols, int64_t n_rows, dq_few_result* results,
                                 int64_t* group_counts, uint8_t* group_keys, int32_t* group_lens);

/* ---------------------------------------------------------------- frequency group-by
 * Replaces FrequencyBasedAnalyzer.computeFrequencies (GroupingAnalyzers.scala:53-80) and the
 * group-by of Histogram (Histogram.scala:54-69).  A dq_freq is the device-resident state
 * FrequenciesAndNumRows(frequencies, numRows) (GroupingAnalyzers.scala:124-157): consuming a
 * batch groups its rows (rows with a NULL grouping value are dropped, numRows counts every
 * row); importing groups is FrequenciesAndNumRows.sum (outer join adding counts).  With a filter
 * (dq_freq_set_filter) the state is that of the filtered data: only rows where the filter is TRUE
 * take part, and numRows counts every selected row (a selected row with a NULL key too).
 *
 * Group keys are exchanged in an encoded form: fixed-width columns as little-endian value bytes
 * (1 B bool/int8, 2 B int16, 4 B int32/float32, 8 B int64/float64; floats as raw bits), strings
 * as UTF-8 bytes; with several grouping columns the parts are concatenated in column order and
 * every string part is prefixed with its u32 length.  With DQ_FREQ_NULL_AS_KEY (Histogram), a
 * NULL string is the key "NullValue" and a NULL of any other type is the empty key. */
typedef struct dq_freq dq_freq;

#define DQ_FREQ_NULL_AS_KEY 0x1
/* Few groups or nothing: one key column, grouped only by the few-groups kernel (per-workgroup
 * LDS tables of 1024 keys of at most 15 bytes).  A batch it cannot hold -- more distinct keys, a
 * longer key -- fails dq_freq_consume with DQ_ERR_SPACE, and every later consume fails alike: the
 * caller drops the table.  ColumnProfiler uses it to try every string column as a
 * low-cardinality histogram in pass 1 (no reference counterpart: a speculative schedule of the
 * same aggregations). */
#define DQ_FREQ_FEW_ONLY 0x2

typedef struct dq_freq_summary {
  int64_t num_rows;      /* FrequenciesAndNumRows.numRows: every consumed row          */
  int64_t num_groups;    /* number of groups (CountDistinct, Distinctness numerator)   */
  int64_t num_unique;    /* groups with count == 1 (Uniqueness numerator)              */
  int64_t grouped_rows;  /* sum of the group counts                                    */
  double entropy;        /* sum over groups of -(c/num_rows) ln(c/num_rows)            */
} dq_freq_summary;

typedef struct dq_freq_group {
  int64_t count;
  int64_t key_offset;    /* into the caller's key byte buffer                         */
  int32_t key_len;
  int32_t reserved;
} dq_freq_group;

dq_status dq_freq_create(dq_ctx* ctx, const int32_t* key_columns, int n_keys,
                         const int32_t* column_types, int n_columns, int flags, dq_freq** out);
dq_status dq_freq_destroy(dq_freq* f);
/* Optional: size the table's staging for `rows` more rows before consuming them (e.g. the row
 * count of every partition about to be consumed), so staging is not regrown batch by batch. */
dq_status dq_freq_reserve(dq_freq* f, int64_t rows);
/* Optional: the caller expects at most `groups` groups (e.g. ColumnProfiler's approximate
 * distinct count before its histogram pass, ColumnProfiler.scala:535-557).  A handful of groups
 * is aggregated in LDS per workgroup instead of being staged and sorted. */
dq_status dq_freq_expect_groups(dq_freq* f, int64_t groups);
dq_status dq_freq_reset(dq_freq* f);
/* The table's `where`: every later batch is grouped as data.filter(where) would be (SQL WHERE: a
 * FALSE or NULL verdict drops the row).  The program's column indices are batch column indices,
 * like key_columns; it is validated as a plan validates a `where` (what a plan declines is
 * declined here with the same status and message).  Set on an empty table (DQ_ERR_STATE once it
 * holds rows or groups); dq_freq_reset keeps it.  DQ_ERR_UNSUPPORTED on a DQ_FREQ_NULL_AS_KEY
 * table.  Per batch the evaluation adds one descriptor copy and two small launches (the predicate
 * mask and its fold into the first key column's validity; three with a LIKE / RLIKE, whose match
 * masks come first) on the table's stream, and no host synchronisation of its own: the selected
 * rows are counted on the device and read back with the counters every path reads anyway.  A
 * table without a filter runs exactly what it ran before. */
dq_status dq_freq_set_filter(dq_freq* f, const dq_predicate* where);
dq_status dq_freq_consume(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows);
/* dq_freq_consume of one Arrow batch (dq_plan_consume_arrow's rules; all the batch's columns). */
dq_status dq_freq_consume_arrow(dq_freq* f, const struct ArrowSchema* schema, const struct ArrowArray* array,
                                int flags);
dq_status dq_freq_get_summary(dq_freq* f, dq_freq_summary* out);
/* Number of groups and total encoded key bytes (to size dq_freq_export's buffers). */
dq_status dq_freq_size(dq_freq* f, int64_t* n_groups, int64_t* key_bytes);
/* Every group, in an unspecified order. */
dq_status dq_freq_export(dq_freq* f, dq_freq_group* groups, int64_t max_groups, uint8_t* key_bytes,
                         int64_t key_cap, int64_t* n_out);
/* The most frequent groups for Histogram's top-maxDetailBins (Histogram.scala:79): every group
 * whose count is at least the n-th largest count -- all ties at the cut included, so the caller
 * can apply its own tie order (Spark's rdd.top breaks ties arbitrarily) -- sorted by count
 * descending, then encoded key ascending.  *n_out / *key_bytes_out receive the sizes; when they
 * exceed max_groups / key_cap nothing is written and DQ_ERR_SPACE is returned. */
dq_status dq_freq_top(dq_freq* f, int n, dq_freq_group* groups, int64_t max_groups, uint8_t* key_bytes,
                      int64_t key_cap, int64_t* n_out, int64_t* key_bytes_out);
/* dst += src on the device (FrequenciesAndNumRows.sum, GroupingAnalyzers.scala:128-148): both
 * tables on one device, grouping the same key types; src is unchanged. */
dq_status dq_freq_merge(dq_freq* dst, dq_freq* src);
/* Distance.categoricalDistance over two states (Distance.scala:43-87): linf_simple = the maximum
 * over the union of keys of |ca / n - cb / m| (an absent key counts 0; each quotient one fp64
 * division), bit-equal to the reference.  Exactly one table without groups: NaN (0L / 0.0); both:
 * 0.0.  The tables' preconditions are dq_freq_merge's (a == b is allowed: 0.0); a total above
 * 2^53 is DQ_ERR_UNSUPPORTED (the reference's fp64 sum then depends on its order).  Neither
 * table changes.  selectMetrics' robust variant is the caller's arithmetic on linf_simple, n, m. */
typedef struct dq_freq_distance {
  double  linf_simple;
  int64_t n, m;             /* sums of the group counts of a and of b */
  int64_t groups_a, groups_b, groups_common;
} dq_freq_distance;
dq_status dq_freq_linf_distance(dq_freq* a, dq_freq* b, dq_freq_distance* out);
/* MutualInformation over one state of two key columns (MutualInformation.scala:38-81), on the
 * device: mi = the sum over the joint groups of (pxy / total) * log((pxy / total) / ((px / total) *
 * (py / total))), total = (double)num_rows (rows with a NULL key included), px / py the sums of the
 * joint counts over each value of key column 0 / 1, every operation one IEEE fp64 operation in that
 * order.  The terms are added exactly (128-bit fixed point, 96 fraction bits, each term rounded to
 * nearest-even once) and the sum is rounded to fp64 once, so mi does not depend on the order of
 * the groups: a merged state and the union of its rows give the same bits.  The table must group
 * exactly two key columns (they may be the same column) and not be a DQ_FREQ_NULL_AS_KEY table
 * (DQ_ERR_INVALID).  No groups: DQ_OK, mi = NaN, the group counts 0.  A group of count 0 makes its
 * term 0 * -inf or log(NaN): mi = NaN, as on the JVM.  num_rows above 2^53, or below the sum of
 * the counts, is DQ_ERR_UNSUPPORTED.  The table does not change. */
typedef struct dq_freq_mi {
  double  mi;         /* sum over the joint groups                                */
  int64_t num_rows;   /* the state's numRows (`total` of the reference)           */
  int64_t groups;     /* joint groups                                             */
  int64_t groups_a;   /* distinct values of key column 0 among the groups         */
  int64_t groups_b;   /* ... of key column 1                                      */
} dq_freq_mi;
dq_status dq_freq_mutual_information(dq_freq* f, dq_freq_mi* out);
/* Merge groups (and `num_rows`) into the table: FrequenciesAndNumRows.sum. */
/* Count of one group (0 if the key is absent), key in the encoded form above.  Used to fold a
 * literal "NullValue" string into Histogram's NULL bin when Histogram shares the frequency
 * table of its column (Histogram.scala:63-64: NULL is replaced by that literal before grouping). */
dq_status dq_freq_lookup(dq_freq* f, const uint8_t* key, int64_t key_len, int64_t* count);
dq_status dq_freq_import(dq_freq* f, const dq_freq_group* groups, int64_t n, const uint8_t* key_bytes,
                         int64_t num_rows);

/* ---- Columnar (Arrow-layout) state interchange: FrequenciesAndNumRows.frequencies as the
 * DataFrame columns HdfsStateProvider persists (StateProvider.scala:222-240) and loads
 * (:280-311), with no per-group record anywhere.  Group i = (counts[i], the encoded key
 * key_bytes[key_offsets[i] .. key_offsets[i + 1])); key_offsets holds n + 1 values (Arrow's
 * large-offset layout).  DQ_FLAT_DEVICE: the three buffers are device memory on the table's
 * device, else host memory. */
#define DQ_FLAT_DEVICE 0x1
/* Every group in slot order (the same table exports the same columns).  *n_out / *key_bytes_out
 * receive the sizes; when they exceed max_groups / key_cap (or a buffer is NULL) nothing is
 * written and DQ_ERR_SPACE is returned -- the export stays on the device for the filling call,
 * which hands it over. */
dq_status dq_freq_export_flat(dq_freq* f, int64_t* counts, int64_t* key_offsets, uint8_t* key_bytes,
                              int64_t max_groups, int64_t key_cap, int flags, int64_t* n_out, int64_t* key_bytes_out);
/* FrequenciesAndNumRows.sum of n flat groups (+ num_rows): duplicate keys add up, as the
 * reference's outer join does (GroupingAnalyzers.scala:128-148).  Offsets are validated first. */
dq_status dq_freq_import_flat(dq_freq* f, const int64_t* counts, const int64_t* key_offsets, const uint8_t* key_bytes,
                              int64_t n, int64_t num_rows, int flags);

/* ---------------------------------------------------------------- multi-GPU key-hash exchange
 * The frequency family's one real exchange step: Spark shuffles the partial
 * group counts by key hash into spark.sql.shuffle.partitions before the final aggregate
 * (GroupingAnalyzers.scala:67-72).  Here every rank partitions its local table by owner rank
 * (a hash of the encoded key), the ranks exchange the partitions with one all-to-all (RCCL over
 * xGMI), and every owner merges what it receives with dq_freq_import_parts -- after which the
 * owners hold disjoint keys, and their count-of-counts histograms add up to the global one. */
typedef struct dq_freq_wire {  /* one group in device memory (32 B)                         */
  uint64_t ctrl;               /* key length (low 24 bits) | 1 << 30 if the key is in key bytes */
  int64_t count;
  uint64_t k0, k1;             /* key bytes (<= 16 B, little-endian), or k0 = key-byte offset  */
} dq_freq_wire;

typedef struct dq_freq_wire_packed {  /* a group whose key packs into one word (16 B):        */
  uint64_t key;                       /* a decimal digit string of <= 15 bytes -- nibble i =   */
  int64_t count;                      /* digit i, the length in the top nibble -- or 0xA for   */
} dq_freq_wire_packed;                /* Histogram's "NullValue" group                         */

/* Write every group of `f`, partitioned by owner (0 .. n_parts-1), into DEVICE buffers on f's
 * GPU.  Part p follows parts 0..p-1 in d_out and is part_packed[p] dq_freq_wire_packed records
 * (16 B: keys that pack) then part_groups[p] dq_freq_wire records (32 B: every other key), each
 * section in the order of f's table slices -- so the receiver merges a part slice by slice with
 * no sort.  Long keys (8-byte padded) of part p follow those of parts 0..p-1 in d_key_bytes, k0
 * relative to the start of part p's key region.  The sizes go to the three host arrays (n_parts
 * each); if a buffer is too small nothing is written and DQ_ERR_SPACE is returned (call once with
 * out_bytes = 0 to size them: part p takes 16 part_packed[p] + 32 part_groups[p] bytes).
 * Replaces the map side of the groupBy's hash exchange (GroupingAnalyzers.scala:67-72). */
dq_status dq_freq_partition(dq_freq* f, int n_parts, void* d_out, int64_t out_bytes, uint8_t* d_key_bytes,
                            int64_t key_cap, int64_t* part_packed, int64_t* part_groups,
                            int64_t* part_key_bytes);
/* Merge the parts other ranks partitioned for this one (laid out as dq_freq_partition writes
 * them, one after the other in d_parts / d_key_bytes) into f: each of f's slices is merged once,
 * in LDS, from the matching records of every part (FrequenciesAndNumRows.sum's outer join,
 * GroupingAnalyzers.scala:128-148); num_rows is added to numRows. */
dq_status dq_freq_import_parts(dq_freq* f, int n_parts, const void* d_parts, const int64_t* part_packed,
                               const int64_t* part_groups, const uint8_t* d_key_bytes,
                               const int64_t* part_key_bytes, int64_t num_rows);
/* Merge n general groups held in DEVICE memory (dq_freq_wire, any order) into f. */
dq_status dq_freq_import_wire(dq_freq* f, const dq_freq_wire* d_groups, int64_t n,
                              const uint8_t* d_key_bytes, int64_t key_bytes, int64_t num_rows);
/* Count-of-counts of f: hist[c] = number of groups with count c (1 <= c < n_bins, hist[0] = 0);
 * counts >= n_bins go to big[] ascending (*n_big; DQ_ERR_SPACE if big_cap is too small). */
dq_status dq_freq_count_histogram(dq_freq* f, int64_t* hist, int64_t n_bins, int64_t* big,
                                  int64_t big_cap, int64_t* n_big);
/* The dq_freq_summary of a (summed) count-of-counts histogram and numRows, with the same fixed
 * summation order as dq_freq_get_summary. */
dq_status dq_freq_summary_from_histogram(const int64_t* hist, int64_t n_bins, const int64_t* big,
                                         int64_t n_big, int64_t num_rows, dq_freq_summary* out);

/* ---------------------------------------------------------------- multi-GPU groups (RCCL)
 * One process (or one JVM executor thread) per GPU, each with its own dq_ctx, joined into a
 * dq_group -- an RCCL communicator over xGMI -- so that a driver that is not torch (the JNI shim)
 * can run the sharded path.  Each rank scans its own row shard; the group then
 * replaces Spark's final aggregation (AnalysisRunner.scala:313: partial states of every partition
 * merged by the aggregate) and the shuffle of the frequency family (GroupingAnalyzers.scala:
 * 67-72).  Every dq_group_* call is collective: all ranks call it in the same order. */
typedef struct dq_group dq_group;

#define DQ_GROUP_ID_BYTES 128

/* A fresh group id on the rank that creates the group (ncclGetUniqueId); the caller ships the
 * bytes to every other rank (e.g. through the Spark driver) before dq_group_create. */
dq_status dq_group_unique_id(uint8_t id[DQ_GROUP_ID_BYTES]);
dq_status dq_group_create(dq_ctx* ctx, int n_ranks, int rank, const uint8_t id[DQ_GROUP_ID_BYTES],
                          dq_group** out);
dq_status dq_group_destroy(dq_group* g);

/* In place: states[0..n_ops) of this rank's shard become those of the whole dataset -- ONE
 * all-gather of the POD states over RCCL, then the fold in rank order of dq_states_merge_ranks
 * (deterministic: every rank computes the same bytes). */
dq_status dq_group_allgather_merge(dq_group* g, dq_state* states, int n_ops);

/* The fold dq_group_allgather_merge applies (host only): gathered = n_ranks blocks of n_ops
 * states in rank order; out[i] = Analyzers.merge of gathered[r * n_ops + i] over r = 0, 1, ...
 * (State.sum per kind, Analyzer.scala:367-386; e.g. StandardDeviation.scala:37-44). */
dq_status dq_states_merge_ranks(const dq_state* gathered, int n_ranks, int n_ops, dq_state* out);

/* Every dq_group_* call is collective; a failure of any rank's local step fails the call on
 * every rank (agreed on before data moves), so no rank is left blocked in a collective.
 *
 * The key-hash exchange: every rank partitions `local` by owner (dq_freq_partition), the parts
 * travel in one RCCL all-to-all (grouped send/recv), and each rank merges what it receives into
 * `owned` (an empty table with the same key columns) -- which then holds the keys this rank owns,
 * disjoint across ranks.  *num_rows = the dataset's numRows (sum over ranks). */
dq_status dq_group_freq_exchange(dq_group* g, dq_freq* local, dq_freq* owned, int64_t* num_rows);

/* dq_freq_summary of the whole dataset from the owned tables: the count-of-counts histograms
 * all-reduced (sum) over RCCL, counts beyond the histogram all-gathered, then the fixed-order
 * dq_freq_summary_from_histogram -- equal, bit for bit, to a single table over all rows. */
dq_status dq_group_freq_summary(dq_group* g, dq_freq* owned, int64_t num_rows, dq_freq_summary* out);

/* Histogram's top-maxDetailBins over the whole dataset (Histogram.scala:78-79, rdd.top + the
 * groupBy's exchange): the union of every owner's dq_freq_top(owned, n), cut at the n-th largest
 * count with all ties kept, count descending then encoded key ascending -- dq_freq_top's contract
 * over the union of the ranks' rows.  Same buffer protocol as dq_freq_top: on DQ_ERR_SPACE
 * *n_out / *key_bytes_out hold the sizes and every rank retries with larger buffers. */
dq_status dq_group_freq_top(dq_group* g, dq_freq* owned, int n, dq_freq_group* groups, int64_t max_groups,
                            uint8_t* key_bytes, int64_t key_cap, int64_t* n_out, int64_t* key_bytes_out);

/* ---------------------------------------------------------------- KLL sketches
 * KLLSketch (KLLSketch.scala:90-170) has a runner of its own in the reference
 * (KLLRunner.computeKLLSketchesInExtraPass, KLLRunner.scala:89-122) and a state of variable size
 * (QuantileNonSample[Double] + globalMax / globalMin), so it has a small family here rather than a
 * dq_op.  The reference's sketch is deterministic; its result depends only on the partitioning, which
 * this library fixes (KLLSketch): a batch is cut into slabs of `slab_rows` consecutive
 * rows, each slab is sketched as one reference partition (KLLRunner.scala:150-177), the slabs of a
 * batch are merged by a balanced tree in slab order with QuantileNonSample.merge, and batches are
 * merged in arrival order (KLLState.sum).  The result is a pure function of the rows, the parameters
 * and slab_rows.
 *
 * Call sequence: dq_kll_create, dq_kll_consume per batch (synchronous), dq_kll_finish for the export
 * sizes, dq_kll_export per sketched column, dq_kll_destroy.  Not thread-safe. */
typedef struct dq_kll dq_kll;

typedef struct dq_kll_column {
  int32_t column;           /* batch column index: INT8..INT64, FLOAT32, FLOAT64          */
  int32_t sketch_size;      /* KLLParameters.sketchSize (default 2048)                     */
  double shrinking_factor;  /* KLLParameters.shrinkingFactor (default 0.64)                */
} dq_kll_column;

/* DQ_OK when the GPU sketcher takes these parameters.  DQ_ERR_UNSUPPORTED (dq_last_error names
 * the bound) when the capacity of the sketch's levels exceeds what a workgroup's LDS holds, e.g.
 * sketchSize 50000 or a shrinking factor >= 1: the caller sketches on Spark. */
dq_status dq_kll_supported(int32_t sketch_size, double shrinking_factor);

/* slab_rows = 0 selects the library's constant (65536 rows). */
dq_status dq_kll_create(dq_ctx* ctx, const dq_kll_column* columns, int n, const int32_t* column_types,
                        int n_columns, int64_t slab_rows, dq_kll** out);
dq_status dq_kll_consume(dq_kll* k, const dq_column* columns, int n_columns, int64_t n_rows);
/* sizes[i] = bytes dq_kll_export needs for sketched column i.  Without a consumed batch every
 * sketch is empty (min = Int.MaxValue, max = Int.MinValue, KLLRunner.scala:28-29). */
dq_status dq_kll_finish(dq_kll* k, int64_t* sizes, int n);
/* Sketched column i as 8-byte little-endian words: int64 n_levels, double globalMin, double
 * globalMax, per level {int64 length, int64 numOfCompress, int64 offset}, then the compactors'
 * items (doubles) level by level.  *required = the bytes needed; DQ_ERR_SPACE when `capacity` is
 * smaller (retry with a larger buffer). */
dq_status dq_kll_export(dq_kll* k, int i, void* out, int64_t capacity, int64_t* required);
dq_status dq_kll_destroy(dq_kll* k);

/* ---------------------------------------------------------------- approximate quantiles
 * ApproxQuantile / ApproxQuantiles (ApproxQuantile.scala, ApproxQuantiles.scala) keep a
 * Greenwald-Khanna digest of a numeric column cast to double, NULLs skipped, no `where`.  The
 * reference's digest depends on Spark's partitioning; this library's is a pure function of the rows,
 * relativeError and the batch boundaries (ApproxQuantile): every batch is summarised by
 * the exact values at ranks 1, 1 + gap, ..., n with gap = max(1, floor(relativeError * n)), found on
 * the GPU by a multi-rank radix select, and the batch summaries are merged on the host in arrival
 * order.  One dq_aq serves every (column, relativeError) pair of a run: one launch per pass covers
 * them all.
 *
 * Call sequence: dq_aq_create, dq_aq_consume per batch (synchronous), dq_aq_finish for the export
 * sizes, dq_aq_export per digest, dq_aq_destroy.  Not thread-safe. */
typedef struct dq_aq dq_aq;

typedef struct dq_aq_column {
  int32_t column;         /* a numeric column of the schema   */
  int32_t reserved;
  double relative_error;  /* relativeError (default 0.01)     */
} dq_aq_column;

/* DQ_OK when the GPU select serves this relativeError.  DQ_ERR_UNSUPPORTED, the message naming the
 * bound, for 0 (an exact quantile needs a full sort) and for values below 0.001 (the select keeps at
 * most 2048 target ranks per batch); DQ_ERR_INVALID outside [0, 1]. */
dq_status dq_aq_supported(double relative_error);
/* columns[i]: one digest; column_types[n_columns]: the dq_type of every column of the batches
 * to come. */
dq_status dq_aq_create(dq_ctx* ctx, const dq_aq_column* columns, int n, const int32_t* column_types, int n_columns,
                       dq_aq** out);
/* DQ_ERR_UNSUPPORTED for a batch of more than 2^31 - 1 rows (row counts and gaps are 32-bit). */
dq_status dq_aq_consume(dq_aq* a, const dq_column* columns, int n_columns, int64_t n_rows);
/* sizes[i] = bytes dq_aq_export needs for digest i.  Without a non-NULL value the digest is empty. */
dq_status dq_aq_finish(dq_aq* a, int64_t* sizes, int n);
/* Digest i in its serialised form, every field big-endian: int32 compressThreshold (10000), float64
 * relativeError, int64 count, int32 len, then per entry float64 value, int32 g, int32 delta.
 * *required = the bytes needed; DQ_ERR_SPACE when `capacity` is smaller. */
dq_status dq_aq_export(dq_aq* a, int i, void* out, int64_t capacity, int64_t* required);
dq_status dq_aq_destroy(dq_aq* a);

/* ---------------------------------------------------------------- row-level schema validation
 * RowLevelSchemaValidator.validate (schema/RowLevelSchemaValidator.scala:183-281) on batches of
 * string-typed columns: per row the Kleene AND of the definitions' conjuncts; the TRUE rows are
 * validRows (int definitions cast to int32, decimal definitions to int64 unscaled values, the last
 * definition of a column deciding its cast), the FALSE rows invalidRows (as they came); a row whose
 * conjunction is NULL (a NULL cell of an int definition with a minValue, line 246) is in neither.
 *
 * Call sequence per batch: dq_schema_validate (synchronous: counts and every output's layout are
 * known when it returns), then per wanted output column dq_schema_output_layout and dq_schema_gather
 * into device buffers the caller allocated -- the rows are written once, into memory their owner
 * manages; nothing is left to release.  The input columns of a DQ_COL_DEVICE batch must stay alive
 * until the last dq_schema_gather of that batch.  Outputs are in input row order, Arrow layout,
 * offset 0.  Not thread-safe. */
typedef struct dq_schema dq_schema;

enum { DQ_SCHEMA_STRING = 0, DQ_SCHEMA_INT = 1, DQ_SCHEMA_DECIMAL = 2, DQ_SCHEMA_TIMESTAMP = 3 };
#define DQ_SCHEMA_NOT_NULL 0x1    /* isNullable = false                                     */
#define DQ_SCHEMA_HAS_MIN 0x2     /* min_value is set: minValue (int) / minLength (string)  */
#define DQ_SCHEMA_HAS_MAX 0x4     /* max_value is set: maxValue (int) / maxLength (string)  */
#define DQ_SCHEMA_HAS_PATTERN 0x8 /* pattern is set: matches (string)                       */

typedef struct dq_schema_def {
  int32_t kind;        /* DQ_SCHEMA_*                                          */
  int32_t column;      /* index into column_types                              */
  int32_t flags;       /* DQ_SCHEMA_NOT_NULL | HAS_MIN | HAS_MAX | HAS_PATTERN */
  int32_t precision;   /* decimal                                              */
  int32_t scale;
  int32_t pattern_len;
  int64_t min_value;   /* 32-bit range, as the reference's Option[Int]         */
  int64_t max_value;
  const uint8_t* pattern; /* UTF-8 text of the java.util.regex pattern         */
} dq_schema_def;

/* Compiles the definitions (patterns included, as PatternMatch's are).  DQ_ERR_UNSUPPORTED, with
 * dq_last_error naming the definition: a timestamp definition, a pattern outside the exact regex
 * subset (the compiler's message follows), a definition on a column that is not utf8, decimal
 * precision above 18.  DQ_ERR_INVALID: precision outside 1..38, scale outside 0..precision, a
 * column out of range, a bound outside 32 bits. */
dq_status dq_schema_create(dq_ctx* ctx, const dq_schema_def* defs, int n_defs, const int32_t* column_types,
                           int n_columns, dq_schema** out);
/* The same checks without a device (the status and message dq_schema_create would give). */
dq_status dq_schema_supported(const dq_schema_def* defs, int n_defs, const int32_t* column_types, int n_columns);
/* Validates one batch.  def_flags (n_defs entries, may be NULL): 1 for a decimal definition that met
 * a cell the GPU cannot judge exactly (a byte >= 0x80, an exponent beyond +-1000); the call then
 * returns DQ_ERR_UNSUPPORTED and the batch has no outputs. */
dq_status dq_schema_validate(dq_schema* s, const dq_column* columns, int n_columns, int64_t n_rows,
                             int64_t* num_valid, int64_t* num_invalid, int32_t* def_flags);
/* Output `which` (0 validRows, 1 invalidRows), column `column` of the last batch: its dq_type and
 * the bytes of its three buffers (0 = the buffer is absent; bit buffers are whole 64-bit words;
 * utf8 offsets always hold count + 1 entries). */
dq_status dq_schema_output_layout(dq_schema* s, int which, int column, int32_t* type, int64_t* values_bytes,
                                  int64_t* validity_bytes, int64_t* offsets_bytes);
/* Writes that column into device buffers of those sizes (a buffer of 0 bytes may be NULL).
 * Synchronous. */
dq_status dq_schema_gather(dq_schema* s, int which, int column, void* values, void* validity, void* offsets);
/* The source row of every output row, in row order, to host memory (DQ_ERR_SPACE when capacity,
 * in entries, is below the output's row count). */
dq_status dq_schema_selection(dq_schema* s, int which, int32_t* out, int64_t capacity);
dq_status dq_schema_destroy(dq_schema* s);

/* ---------------------------------------------------------------- row-level outcomes
 * Which rows an analyzer counts.  Every outcome is one nullable boolean per row, held as two device
 * bitmaps in the Arrow boolean layout (LSB first, whole 64-bit words): `value` (bit = TRUE) and
 * `valid` (bit = not NULL).  A row that the op's `where` does not select (FALSE or NULL) is NULL;
 * a selected row is TRUE where
 *   DQ_OP_COMPLETENESS   the column is not NULL,
 *   DQ_OP_COMPLIANCE     the predicate is TRUE (a NULL predicate is FALSE),
 *   DQ_OP_PATTERN_MATCH  the value holds a non-empty match (a NULL value is FALSE),
 *   dq_freq_probe_rows   the row's key has count exactly 1 in the table probed (a NULL key column
 *                        and a key absent from the table are FALSE),
 * so popcount(value) is the numerator and popcount(valid) the denominator of the state the same op
 * (or the table's group-by) yields over the same rows.
 *
 * A batch writes its n_rows outcomes at bit `out_bit_offset` of the caller's bitmaps (its row offset
 * in a bitmap pair that spans several batches): bits [out_bit_offset, out_bit_offset + n_rows).  The
 * other bits of the first and last word touched keep their values, so the caller zeroes the bitmaps
 * once; batches that share a word are evaluated one after the other.  Every call is synchronous. */
typedef struct dq_rows dq_rows;
/* Ops: DQ_OP_COMPLETENESS, DQ_OP_COMPLIANCE, DQ_OP_PATTERN_MATCH (anything else is DQ_ERR_INVALID),
 * each checked as dq_op_supported checks it. */
dq_status dq_rows_create(dq_ctx* ctx, const dq_op* ops, int n_ops, const int32_t* column_types, int n_columns,
                         dq_rows** out);
/* d_value[i] / d_valid[i]: op i's device bitmaps. */
dq_status dq_rows_evaluate(dq_rows* rows, const dq_column* columns, int n_columns, int64_t n_rows,
                           int64_t out_bit_offset, uint64_t* const* d_value, uint64_t* const* d_valid);
dq_status dq_rows_destroy(dq_rows* rows);
/* Probes the table (read only; any staged rows are aggregated first) with the key of every row of
 * the batch, whose columns are the table's.  d_selected (NULL: every row) is a device bitmap at bit
 * 0 of the rows a `where` selects, (n_rows + 63) / 64 words, e.g. the `value` bitmap of a
 * DQ_OP_COMPLIANCE outcome of the filter.  d_counts (NULL: not wanted) receives n_rows counts, 0
 * for a row without a key or with a key the table does not hold, whatever d_selected says.
 * A DQ_FREQ_NULL_AS_KEY table is DQ_ERR_INVALID. */
dq_status dq_freq_probe_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows,
                             const uint64_t* d_selected, int64_t out_bit_offset, uint64_t* d_value,
                             uint64_t* d_valid, int64_t* d_counts);
/* The ascending row indices of the outcomes named by `which` (an OR of DQ_ROWS_*) among the first
 * n_rows bits of a bitmap pair, into the device array d_out; *n_out = how many there are.  When
 * that is above `capacity` (entries) nothing is written and the call returns DQ_ERR_SPACE: a call
 * with capacity 0 counts. */
#define DQ_ROWS_FALSE 1
#define DQ_ROWS_TRUE 2
#define DQ_ROWS_NULL 4
dq_status dq_rows_select(dq_ctx* ctx, const uint64_t* d_value, const uint64_t* d_valid, int64_t n_rows, int which,
                         int64_t* d_out, int64_t capacity, int64_t* n_out);

/* ---------------------------------------------------------------- correlation matrix
 * Every pairwise Correlation(x, y, where) state of up to 64 numeric columns from one pass over the
 * rows: k columns give k (k + 1) / 2 states, i <= j in the order the columns were selected, row-major
 * over the upper triangle (pair (i, j) at i k - i (i - 1) / 2 + (j - i)).  A row counts for (x, y)
 * when x and y are non-NULL and the `where` is TRUE; every value is cast to double as Correlation
 * casts it.  The sums run on the fp64 matrix cores over slabs of 1024 rows; a pair that some slab of
 * a batch cannot answer that way (a selected non-finite value in one of its columns, sums that are
 * not finite, a shift that is an outlier: DESIGN.md, Correlation matrix) takes its state of that
 * batch from the pair kernel of DQ_OP_CORRELATION, over the same rows (finite values whose sums
 * overflow: from Spark's per-row update).  Batches accumulate in call
 * order with CorrelationState.sum; the states are bitwise reproducible on one device.
 *
 * Call sequence: dq_corrmat_create, dq_corrmat_consume per batch (synchronous), dq_corrmat_finish;
 * dq_corrmat_reset starts over with the same columns and filter.  Not thread-safe. */
typedef struct dq_corrmat dq_corrmat;
/* column_types: the batch's schema; columns: the n_selected (1 to 64: more is DQ_ERR_UNSUPPORTED)
 * distinct numeric columns of the matrix; where: the optional filter (NULL or n_insns = 0: none),
 * checked as a dq_op's. */
dq_status dq_corrmat_create(dq_ctx* ctx, const int32_t* column_types, int n_columns, const int32_t* columns,
                            int n_selected, const dq_predicate* where, dq_corrmat** out);
dq_status dq_corrmat_consume(dq_corrmat* m, const dq_column* columns, int n_columns, int64_t n_rows);
/* states: 6 doubles per pair {n, xAvg, yAvg, ck, xMk, yMk}, six zeros for a pair without a row.
 * *fallback_pairs (may be NULL) = the pair-batches answered by the pair kernel so far. */
dq_status dq_corrmat_finish(dq_corrmat* m, double* states, int64_t* fallback_pairs);
dq_status dq_corrmat_reset(dq_corrmat* m);
dq_status dq_corrmat_destroy(dq_corrmat* m);

/* ---------------------------------------------------------------- cross-table checks
 * Referential integrity and dataset match between a primary table A and a reference table B, as
 * row-level outcomes of A (the bitmap pair above).  The dq_freq is the group-by of B's key columns
 * (not a DQ_FREQ_NULL_AS_KEY one: DQ_ERR_INVALID); A's key columns are handed to it in the place of
 * B's (same count, order and types).  A row of A that d_selected does not select is NULL; a
 * selected row is TRUE iff every key column is non-NULL, the table holds the key, and -- with
 * compare pairs -- every pair (a_compare[p], b_compare[p]) is NULL-safe equal between that row of A
 * and the row of B holding the key: NULL equals NULL only; integers, bool and decimal128 by value;
 * float32 / float64 as Spark's doubles (any NaN equals any NaN, -0.0 equals 0.0); strings by length
 * and bytes.  Key equality is the group-by's own.
 *
 * dq_freq_index_rows records, for every row of a batch of B that has a key, which row holds it:
 * row_offset + the row's index in the batch, in an int64 per table slot that the handle owns.  The
 * index lives until the table changes (consume, merge, import, reset), and is built anew by the
 * first call after that.  The batch must be rows the table was built from: a key the table does not
 * hold is DQ_ERR_STATE (and drops the index), a filtered table DQ_ERR_INVALID.  With a key in several
 * rows any one of them stays; dataset match needs unique keys, which dq_freq_get_summary shows
 * (num_groups == num_unique).
 *
 * dq_freq_match_rows writes the outcomes of one batch of A at out_bit_offset, as
 * dq_freq_probe_rows does, and ADDS the batch's rows to *counts (NULL: not wanted): of the selected
 * rows, `matched` are TRUE, `key_null` have a NULL key column, `key_absent` a key the table (or,
 * when the index is followed, its indexed rows) does not hold, `cells_differ` a compare pair that
 * differs; the four sum to the selected rows.  The compare columns are DQ_COL_DEVICE columns of
 * equal type per pair, read in place at their `offset`: a_compare over the batch's n_rows rows,
 * b_compare over all b_rows rows of B (the rows the index numbers).  At most DQ_MATCH_MAX_PAIRS
 * pairs (more: DQ_ERR_UNSUPPORTED).  d_reference_rows (NULL: not wanted) receives, per row of the
 * batch and whatever d_selected says, the row of B holding its key, or -1.  Compare pairs and
 * d_reference_rows follow the index (DQ_ERR_STATE without one); with neither, the index is not
 * needed and not read, so the table may be a loaded or merged state of the reference keys. */
#define DQ_MATCH_MAX_PAIRS 32
typedef struct dq_match_counts {
  int64_t matched, key_null, key_absent, cells_differ;
} dq_match_counts;
dq_status dq_freq_index_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows, int64_t row_offset);
dq_status dq_freq_match_rows(dq_freq* f, const dq_column* columns, int n_columns, int64_t n_rows,
                             const uint64_t* d_selected, int64_t out_bit_offset, uint64_t* d_value, uint64_t* d_valid,
                             const dq_column* a_compare, const dq_column* b_compare, int n_pairs, int64_t b_rows,
                             int64_t* d_reference_rows, dq_match_counts* counts);

/* ---------------------------------------------------------------- take
 * The rows of a table named by row indices, as new columns in buffers the caller owns: what turns
 * the row numbers of dq_rows_select and d_reference_rows into records.  A column is n_chunks
 * DQ_COL_DEVICE dq_columns of one type (the batches of a partitioned table), chunk c holding
 * chunk_rows[c] rows; d_rows (a device array of m int64) numbers the rows of their concatenation
 * from 0, in any order and with repeats.  -1 means "no row": every column's output cell is NULL.
 * Any other value outside [-1, total rows) makes dq_take_create return DQ_ERR_INVALID, with the
 * first offending position and its value in dq_last_error.  The indices are checked, and mapped to
 * (chunk, local row), once, in a pass that reads only d_rows; the handle keeps the map for every
 * column and no longer reads d_rows.  n_chunks is 1..4096 (more: DQ_ERR_UNSUPPORTED); m = 0 is
 * valid and gives empty outputs.
 *
 * Per column: dq_take_layout sizes the output, the caller allocates device buffers of those sizes
 * (0: the buffer is absent and its pointer may be NULL), and dq_take_gather -- with the same
 * chunks -- fills them: Arrow layout at offset 0, in the order of d_rows.  Types: bool, int8..int64,
 * float32, float64, every decimal(p,s) (16-byte cells) and utf8.  A chunk's `offset` is honoured
 * for values, for bit buffers at any bit offset and for utf8 offsets; a utf8 heap need not start at
 * its byte 0.  Bit buffers (bool values, validity) are whole 64-bit words, the bits past m 0, and
 * need 8-byte aligned outputs; value buffers their width's alignment.  validity_bytes is 0 when no
 * chunk has a validity buffer and no index is -1.  A fixed-width NULL cell holds its source's bytes
 * (a -1 cell zeros); a utf8 NULL cell has length 0 whatever offsets the source gives it, and its
 * source bytes are never read.  utf8 output offsets are int32: when the gathered bytes exceed
 * INT32_MAX, dq_take_layout returns DQ_ERR_SPACE with the total in dq_last_error (the lengths are
 * summed in 64 bits) before any byte is copied.  A host-resident chunk, a chunk of another type
 * or row count is DQ_ERR_INVALID.  Calls are synchronous and, per handle, not thread-safe. */
typedef struct dq_take dq_take;
dq_status dq_take_create(dq_ctx* ctx, const int64_t* d_rows, int64_t m, const int64_t* chunk_rows, int n_chunks,
                         dq_take** out);
/* *n_null_rows = how many of the m indices are -1. */
dq_status dq_take_info(dq_take* take, int64_t* n_null_rows);
dq_status dq_take_layout(dq_take* take, const dq_column* chunks, int32_t* type, int64_t* values_bytes,
                         int64_t* validity_bytes, int64_t* offsets_bytes);
/* The column dq_take_layout was last called for (anything else: DQ_ERR_STATE). */
dq_status dq_take_gather(dq_take* take, const dq_column* chunks, void* values, void* validity, void* offsets);
dq_status dq_take_destroy(dq_take* take);

#ifdef __cplusplus
}
#endif
#endif /* DEEQU_AMD_H */
