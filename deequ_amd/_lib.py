"""ctypes binding of the deequ_amd C-ABI (include/deequ_amd.h).

The shared library is built in-tree (`deequ_amd/libdeequ_amd.so`, see
`deequ_amd/csrc/Makefile` / `__graft_entry__.build()`).  There is no fallback: if the
library is missing, importing the compute entry points raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t,
                    c_uint8, c_uint64, c_void_p)

# DEEQU_AMD_LIB points at another build of the same library (A/B kernel experiments in one run)
LIB_PATH = os.environ.get("DEEQU_AMD_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "libdeequ_amd.so")

# ---------------------------------------------------------------- enums (mirror the header)
DQ_OK, DQ_ERR_INVALID, DQ_ERR_UNSUPPORTED, DQ_ERR_DEVICE, DQ_ERR_OOM, DQ_ERR_STATE, DQ_ERR_SPACE = range(7)

DQ_T_BOOL, DQ_T_INT8, DQ_T_INT16, DQ_T_INT32, DQ_T_INT64, DQ_T_FLOAT32, DQ_T_FLOAT64, DQ_T_UTF8 = range(1, 9)
DQ_T_DECIMAL128 = 9
DQ_COL_DEVICE = 0x1

(DQ_OP_SIZE, DQ_OP_COMPLETENESS, DQ_OP_COMPLIANCE, DQ_OP_SUM, DQ_OP_MEAN, DQ_OP_STDDEV,
 DQ_OP_MINIMUM, DQ_OP_MAXIMUM, DQ_OP_APPROX_COUNT_DISTINCT, DQ_OP_DATATYPE, DQ_OP_MIN_LENGTH,
 DQ_OP_MAX_LENGTH, DQ_OP_CORRELATION, DQ_OP_PATTERN_MATCH) = range(1, 15)

DQ_P_COLUMN, DQ_P_LIT_INT, DQ_P_LIT_FLOAT, DQ_P_LIT_NULL, DQ_P_COALESCE, DQ_P_LIT_STRING = 1, 2, 3, 4, 5, 6
DQ_P_CAST_DOUBLE = 7
DQ_P_CAST = 8  # arg = target dq_type (TYPE_CODES)
DQ_P_EQ, DQ_P_NE, DQ_P_LT, DQ_P_LE, DQ_P_GT, DQ_P_GE, DQ_P_EQ_NULLSAFE = 10, 11, 12, 13, 14, 15, 16
DQ_P_IS_NULL, DQ_P_IS_NOT_NULL = 20, 21
DQ_P_AND, DQ_P_OR, DQ_P_NOT, DQ_P_TRUE, DQ_P_FALSE = 30, 31, 32, 33, 34
DQ_P_LIKE, DQ_P_RLIKE = 40, 41  # Like / RLike(utf8 column, string literal)
DQ_CMP_AS_INT64, DQ_CMP_AS_FLOAT64 = 0, 1

DQ_HLL_NUM_WORDS = 52
DQ_FREQ_NULL_AS_KEY = 0x1
DQ_FREQ_FEW_ONLY = 0x2
DQ_FLAT_DEVICE = 0x1
DQ_ROWS_FALSE, DQ_ROWS_TRUE, DQ_ROWS_NULL = 1, 2, 4

import re as _re

_DECIMAL_RE = _re.compile(r"^decimal\((\d+),(\d+)\)$")


def decimal_type(precision: int, scale: int) -> int:
    """DQ_T_DECIMAL(p, s): the int32 type code of a decimal column (include/deequ_amd.h)."""
    return DQ_T_DECIMAL128 | (int(precision) << 8) | (int(scale) << 16)


def decimal_params(dtype):
    """(precision, scale) of the dtype string "decimal(p,s)" with precision 1..38 and scale 0..p,
    else None."""
    m = _DECIMAL_RE.match(dtype) if isinstance(dtype, str) else None
    if not m:
        return None
    p, s = int(m.group(1)), int(m.group(2))
    return (p, s) if 1 <= p <= 38 and s <= p else None


def is_decimal(dtype) -> bool:
    return decimal_params(dtype) is not None


class _TypeCodes(dict):
    """dtype string -> dq type code: the eight fixed names, and "decimal(p,s)" parsed on lookup."""

    def __missing__(self, dtype):
        ps = decimal_params(dtype)
        if ps is None:
            raise KeyError(dtype)
        return decimal_type(*ps)

    def __contains__(self, dtype):
        return dict.__contains__(self, dtype) or is_decimal(dtype)


TYPE_CODES = _TypeCodes({
    "bool": DQ_T_BOOL, "int8": DQ_T_INT8, "int16": DQ_T_INT16, "int32": DQ_T_INT32,
    "int64": DQ_T_INT64, "float32": DQ_T_FLOAT32, "float64": DQ_T_FLOAT64, "string": DQ_T_UTF8,
})


class NumericTypes(tuple):
    """The dtypes Preconditions.isNumeric accepts (Analyzer.scala:336): the six fixed names and
    every "decimal(p,s)"."""

    def __contains__(self, dtype):
        return tuple.__contains__(self, dtype) or is_decimal(dtype)


class DqColumn(Structure):
    _fields_ = [("type", c_int32), ("flags", c_int32), ("length", c_int64), ("offset", c_int64),
                ("validity", c_void_p), ("values", c_void_p), ("offsets", c_void_p)]


class DqPredInsn(Structure):
    _fields_ = [("opcode", c_int32), ("arg", c_int32), ("i64", c_int64), ("f64", c_double)]


class DqPredicate(Structure):
    _fields_ = [("code", POINTER(DqPredInsn)), ("n_insns", c_int32), ("strings_len", c_int32),
                ("strings", c_void_p)]


class DqOp(Structure):
    _fields_ = [("kind", c_int32), ("column", c_int32), ("column2", c_int32), ("reserved", c_int32),
                ("predicate", DqPredicate), ("where", DqPredicate)]


class DqState(Structure):
    _fields_ = [("kind", c_int32), ("has_value", c_int32), ("num_matches", c_int64),
                ("count", c_int64), ("sum", c_double), ("n", c_double), ("avg", c_double),
                ("m2", c_double), ("value", c_double), ("words", c_int64 * DQ_HLL_NUM_WORDS),
                ("y_avg", c_double), ("ck", c_double), ("x_mk", c_double), ("y_mk", c_double)]


DQ_FEW_MAX_GROUPS = 1024


class DqFewResult(Structure):
    _fields_ = [("ok", c_int32), ("n_groups", c_int32), ("n_nulls", c_int64),
                ("completeness", DqState), ("hll", DqState), ("dtype", DqState)]


class DqFreqSummary(Structure):
    _fields_ = [("num_rows", c_int64), ("num_groups", c_int64), ("num_unique", c_int64),
                ("grouped_rows", c_int64), ("entropy", c_double)]


class DqFreqDistance(Structure):
    _fields_ = [("linf_simple", c_double), ("n", c_int64), ("m", c_int64), ("groups_a", c_int64),
                ("groups_b", c_int64), ("groups_common", c_int64)]


class DqMatchCounts(Structure):
    _fields_ = [("matched", c_int64), ("key_null", c_int64), ("key_absent", c_int64), ("cells_differ", c_int64)]


class DqFreqMi(Structure):
    _fields_ = [("mi", c_double), ("num_rows", c_int64), ("groups", c_int64), ("groups_a", c_int64),
                ("groups_b", c_int64)]


class DqFreqWire(Structure):
    _fields_ = [("ctrl", c_uint64), ("count", c_int64), ("k0", c_uint64), ("k1", c_uint64)]


class DqFreqGroup(Structure):
    _fields_ = [("count", c_int64), ("key_offset", c_int64), ("key_len", c_int32),
                ("reserved", c_int32)]


class DqKllColumn(Structure):
    _fields_ = [("column", c_int32), ("sketch_size", c_int32), ("shrinking_factor", c_double)]


class DqAqColumn(Structure):
    _fields_ = [("column", c_int32), ("reserved", c_int32), ("relative_error", c_double)]


DQ_SCHEMA_STRING, DQ_SCHEMA_INT, DQ_SCHEMA_DECIMAL, DQ_SCHEMA_TIMESTAMP = range(4)
DQ_SCHEMA_NOT_NULL, DQ_SCHEMA_HAS_MIN, DQ_SCHEMA_HAS_MAX, DQ_SCHEMA_HAS_PATTERN = 1, 2, 4, 8


class DqSchemaDef(Structure):
    _fields_ = [("kind", c_int32), ("column", c_int32), ("flags", c_int32), ("precision", c_int32),
                ("scale", c_int32), ("pattern_len", c_int32), ("min_value", c_int64), ("max_value", c_int64),
                ("pattern", c_char_p)]


class ArrowSchema(Structure):
    """struct ArrowSchema of the Arrow C Data Interface (include/deequ_amd.h)."""


ArrowSchema._fields_ = [("format", c_char_p), ("name", c_char_p), ("metadata", c_char_p), ("flags", c_int64),
                        ("n_children", c_int64), ("children", POINTER(POINTER(ArrowSchema))),
                        ("dictionary", POINTER(ArrowSchema)), ("release", c_void_p), ("private_data", c_void_p)]


class ArrowArray(Structure):
    """struct ArrowArray of the Arrow C Data Interface."""


ArrowArray._fields_ = [("length", c_int64), ("null_count", c_int64), ("offset", c_int64), ("n_buffers", c_int64),
                       ("n_children", c_int64), ("buffers", POINTER(c_void_p)),
                       ("children", POINTER(POINTER(ArrowArray))), ("dictionary", POINTER(ArrowArray)),
                       ("release", c_void_p), ("private_data", c_void_p)]


# measurement entry points (include/deequ_amd_diag.h; not part of the drop-in boundary)
DIAG_SIGNATURES = {
    "dq_diag_hash_rate": (c_int, [c_int, c_int, c_int, POINTER(c_double)]),
    "dq_diag_freq_paths": (c_int, [c_void_p, POINTER(c_int64)]),
    "dq_diag_freq_test_flags": (c_int, [c_void_p, c_int32]),
    "dq_diag_parse_double": (c_int, [c_char_p, c_int64, POINTER(c_double), POINTER(c_int32)]),
    "dq_diag_table_hash": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dq_diag_key_pack": (c_int, [c_char_p, c_int32, POINTER(c_uint64), c_char_p, POINTER(c_int32), POINTER(c_int32)]),
    "dq_diag_uuid_pack": (c_int, [c_char_p, c_int32, POINTER(c_uint64), c_char_p, POINTER(c_int32)]),
    "dq_diag_eval_predicate": (c_int, [POINTER(DqPredicate), POINTER(DqColumn), c_int, c_int64, c_void_p]),
    "dq_diag_cell_equal": (c_int, [POINTER(DqColumn), c_int64, POINTER(DqColumn), c_int64, POINTER(c_int32)]),
    "dq_diag_regex_match": (c_int, [c_char_p, c_int32, c_char_p, c_int64, POINTER(c_int32), POINTER(c_int32),
                                    POINTER(c_int32)]),
    "dq_diag_regex_match_mode": (c_int, [c_char_p, c_int32, c_int32, c_char_p, c_int64, POINTER(c_int32),
                                         POINTER(c_int32), POINTER(c_int32), c_void_p, c_int64, POINTER(c_int64)]),
    "dq_diag_plan_match_tasks": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32)]),
    "dq_diag_kll_sketch": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_double, c_int64, c_void_p, c_int64,
                                   POINTER(c_int64)]),
    "dq_diag_schema_cell": (c_int, [c_int32, c_char_p, c_int64, c_int32, c_int32, POINTER(c_int32),
                                    POINTER(c_int64)]),
    "dq_diag_decimal_to_double": (c_int, [c_uint64, c_int64, c_int32, POINTER(c_double), POINTER(c_int32)]),
    "dq_diag_decimal_bytes": (c_int, [c_uint64, c_int64, c_char_p, POINTER(c_int32)]),
    "dq_diag_mi_split": (c_int, [c_char_p, c_int64, c_int32, c_int32, POINTER(c_int32)]),
    "dq_diag_mi_to_fixed": (c_int, [c_double, POINTER(c_uint64), POINTER(c_int64)]),
    "dq_diag_mi_from_fixed": (c_int, [c_uint64, c_int64, POINTER(c_double)]),
    "dq_diag_plan_groups": (c_int, [c_void_p, POINTER(c_int64), c_int32, POINTER(c_int32), POINTER(c_int64)]),
    "dq_diag_plan_lanemask": (c_int, [c_void_p, POINTER(c_int32), c_int32, POINTER(c_int32)]),
    "dq_diag_take_constants": (c_int, [POINTER(c_int64)]),
    "dq_diag_corrmat_host": (c_int, [POINTER(c_void_p), POINTER(c_void_p), c_void_p, c_int32, c_int64, c_int64,
                                     c_void_p, c_void_p]),
}


# every symbol include/deequ_amd.h declares, with its ctypes signature
SIGNATURES = {
    "dq_last_error": (c_char_p, []),
    "dq_abi_version": (c_int, []),
    "dq_device_count": (c_int, [POINTER(c_int)]),
    "dq_release_cached_memory": (c_int, [c_int]),
    "dq_ctx_create": (c_int, [c_int, c_int, POINTER(c_void_p)]),
    "dq_ctx_destroy": (c_int, [c_void_p]),
    "dq_plan_create": (c_int, [c_void_p, POINTER(DqOp), c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "dq_plan_destroy": (c_int, [c_void_p]),
    "dq_plan_create_packed": (c_int, [c_void_p, c_char_p, c_size_t, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "dq_op_supported": (c_int, [POINTER(DqOp), POINTER(c_int32), c_int]),
    "dq_plan_consume": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64]),
    "dq_plan_finish": (c_int, [c_void_p, POINTER(DqState), c_int]),
    "dq_plan_reset": (c_int, [c_void_p]),
    "dq_host_register": (c_int, [c_void_p, c_size_t]),
    "dq_host_unregister": (c_int, [c_void_p]),
    "dq_arrow_columns": (c_int, [POINTER(ArrowSchema), POINTER(ArrowArray), c_int, POINTER(c_int32),
                                 POINTER(DqColumn), c_int, POINTER(c_int), POINTER(c_int64)]),
    "dq_plan_consume_arrow": (c_int, [c_void_p, POINTER(ArrowSchema), POINTER(ArrowArray), c_int]),
    "dq_freq_consume_arrow": (c_int, [c_void_p, POINTER(ArrowSchema), POINTER(ArrowArray), c_int]),
    "dq_plan_op_status": (c_int, [c_void_p, c_int]),
    "dq_plan_stream": (c_void_p, [c_void_p]),
    "dq_state_merge": (c_int, [POINTER(DqState), POINTER(DqState), POINTER(DqState)]),
    "dq_state_metric": (c_int, [POINTER(DqState), POINTER(c_double)]),
    "dq_hll_count": (c_double, [POINTER(c_int64)]),
    "dq_hll_merge": (None, [POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "dq_hll_words_to_bytes": (None, [POINTER(c_int64), POINTER(c_uint8)]),
    "dq_hll_words_from_bytes": (None, [POINTER(c_uint8), POINTER(c_int64)]),
    "dq_xxh64": (c_uint64, [c_void_p, c_size_t, c_uint64]),
    "dq_freq_create": (c_int, [c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), c_int, c_int,
                               POINTER(c_void_p)]),
    "dq_freq_destroy": (c_int, [c_void_p]),
    "dq_freq_reset": (c_int, [c_void_p]),
    "dq_freq_set_filter": (c_int, [c_void_p, POINTER(DqPredicate)]),
    "dq_freq_consume": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64]),
    "dq_freq_get_summary": (c_int, [c_void_p, POINTER(DqFreqSummary)]),
    "dq_freq_size": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "dq_freq_export": (c_int, [c_void_p, POINTER(DqFreqGroup), c_int64, c_void_p, c_int64,
                               POINTER(c_int64)]),
    "dq_freq_reserve": (c_int, [c_void_p, c_int64]),
    "dq_freq_expect_groups": (c_int, [c_void_p, c_int64]),
    "dq_freq_lookup": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int64)]),
    "dq_freq_top": (c_int, [c_void_p, c_int, POINTER(DqFreqGroup), c_int64, c_void_p, c_int64,
                            POINTER(c_int64), POINTER(c_int64)]),
    "dq_freq_merge": (c_int, [c_void_p, c_void_p]),
    "dq_freq_linf_distance": (c_int, [c_void_p, c_void_p, POINTER(DqFreqDistance)]),
    "dq_freq_mutual_information": (c_int, [c_void_p, POINTER(DqFreqMi)]),
    "dq_freq_import": (c_int, [c_void_p, POINTER(DqFreqGroup), c_int64, c_void_p, c_int64]),
    "dq_freq_export_flat": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                    POINTER(c_int64), POINTER(c_int64)]),
    "dq_freq_import_flat": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int]),
    "dq_cast_utf8": (c_int, [c_void_p, POINTER(DqColumn), c_int64, c_int32, c_void_p, c_void_p, POINTER(c_int64)]),
    "dq_cast_decimal": (c_int, [c_void_p, POINTER(DqColumn), c_int64, c_void_p, c_void_p]),
    "dq_cast_utf8_batch": (c_int, [c_void_p, c_int32, POINTER(DqColumn), c_int64, POINTER(c_int32),
                                   POINTER(c_void_p), POINTER(c_void_p)]),
    "dq_profile_few_strings": (c_int, [c_void_p, c_int32, POINTER(DqColumn), c_int64, POINTER(DqFewResult),
                                       c_void_p, c_void_p, c_void_p]),
    "dq_profile_string_groups": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                         POINTER(DqState), POINTER(DqState)]),
    "dq_freq_partition": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64),
                                  POINTER(c_int64), POINTER(c_int64)]),
    "dq_freq_import_parts": (c_int, [c_void_p, c_int, c_void_p, POINTER(c_int64), POINTER(c_int64), c_void_p,
                                     POINTER(c_int64), c_int64]),
    "dq_freq_import_wire": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64]),
    "dq_freq_count_histogram": (c_int, [c_void_p, POINTER(c_int64), c_int64, POINTER(c_int64), c_int64,
                                        POINTER(c_int64)]),
    "dq_freq_summary_from_histogram": (c_int, [POINTER(c_int64), c_int64, POINTER(c_int64), c_int64, c_int64,
                                               POINTER(DqFreqSummary)]),
    "dq_group_unique_id": (c_int, [POINTER(c_uint8)]),
    "dq_group_create": (c_int, [c_void_p, c_int, c_int, POINTER(c_uint8), POINTER(c_void_p)]),
    "dq_group_destroy": (c_int, [c_void_p]),
    "dq_group_allgather_merge": (c_int, [c_void_p, POINTER(DqState), c_int]),
    "dq_states_merge_ranks": (c_int, [POINTER(DqState), c_int, c_int, POINTER(DqState)]),
    "dq_group_freq_exchange": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    "dq_group_freq_summary": (c_int, [c_void_p, c_void_p, c_int64, POINTER(DqFreqSummary)]),
    "dq_group_freq_top": (c_int, [c_void_p, c_void_p, c_int, POINTER(DqFreqGroup), c_int64, c_void_p, c_int64,
                                  POINTER(c_int64), POINTER(c_int64)]),
    "dq_kll_supported": (c_int, [c_int32, c_double]),
    "dq_kll_create": (c_int, [c_void_p, POINTER(DqKllColumn), c_int, POINTER(c_int32), c_int, c_int64,
                              POINTER(c_void_p)]),
    "dq_kll_consume": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64]),
    "dq_kll_finish": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "dq_kll_export": (c_int, [c_void_p, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "dq_kll_destroy": (c_int, [c_void_p]),
    "dq_aq_supported": (c_int, [c_double]),
    "dq_aq_create": (c_int, [c_void_p, POINTER(DqAqColumn), c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "dq_aq_consume": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64]),
    "dq_aq_finish": (c_int, [c_void_p, POINTER(c_int64), c_int]),
    "dq_aq_export": (c_int, [c_void_p, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "dq_aq_destroy": (c_int, [c_void_p]),
    "dq_schema_create": (c_int, [c_void_p, POINTER(DqSchemaDef), c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "dq_schema_supported": (c_int, [POINTER(DqSchemaDef), c_int, POINTER(c_int32), c_int]),
    "dq_schema_validate": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64, POINTER(c_int64), POINTER(c_int64),
                                   POINTER(c_int32)]),
    "dq_schema_output_layout": (c_int, [c_void_p, c_int, c_int, POINTER(c_int32), POINTER(c_int64),
                                        POINTER(c_int64), POINTER(c_int64)]),
    "dq_schema_gather": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dq_schema_selection": (c_int, [c_void_p, c_int, c_void_p, c_int64]),
    "dq_schema_destroy": (c_int, [c_void_p]),
    "dq_rows_create": (c_int, [c_void_p, POINTER(DqOp), c_int, POINTER(c_int32), c_int, POINTER(c_void_p)]),
    "dq_rows_evaluate": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64, c_int64, POINTER(c_void_p),
                                 POINTER(c_void_p)]),
    "dq_rows_destroy": (c_int, [c_void_p]),
    "dq_freq_probe_rows": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_void_p]),
    "dq_rows_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, POINTER(c_int64)]),
    "dq_freq_index_rows": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64, c_int64]),
    "dq_freq_match_rows": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                   POINTER(DqColumn), POINTER(DqColumn), c_int, c_int64, c_void_p,
                                   POINTER(DqMatchCounts)]),
    "dq_take_create": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int64), c_int, POINTER(c_void_p)]),
    "dq_take_info": (c_int, [c_void_p, POINTER(c_int64)]),
    "dq_take_layout": (c_int, [c_void_p, POINTER(DqColumn), POINTER(c_int32), POINTER(c_int64), POINTER(c_int64),
                               POINTER(c_int64)]),
    "dq_take_gather": (c_int, [c_void_p, POINTER(DqColumn), c_void_p, c_void_p, c_void_p]),
    "dq_take_destroy": (c_int, [c_void_p]),
    "dq_corrmat_create": (c_int, [c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), c_int, POINTER(DqPredicate),
                                  POINTER(c_void_p)]),
    "dq_corrmat_consume": (c_int, [c_void_p, POINTER(DqColumn), c_int, c_int64]),
    "dq_corrmat_finish": (c_int, [c_void_p, c_void_p, POINTER(c_int64)]),
    "dq_corrmat_reset": (c_int, [c_void_p]),
    "dq_corrmat_destroy": (c_int, [c_void_p]),
}

_lib = None


class DeequAmdError(RuntimeError):
    """A non-OK dq_status from the C-ABI (message from dq_last_error)."""

    def __init__(self, status: int, message: str):
        super().__init__("deequ_amd status %d: %s" % (status, message))
        self.status = status


class UnsupportedOnGpu(DeequAmdError):
    """DQ_ERR_UNSUPPORTED: the reference would run this analyzer on Spark instead."""


def lib():
    """Load libdeequ_amd.so (raises if it has not been built -- there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("deequ_amd native library not built: %s (run "
                              "`python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Only one
        # HIP runtime can live in a process; whichever is loaded first serves everyone, and
        # torch cannot run on a newer one.  So when torch is installed, let it load its runtime
        # first and bind this library to that same runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(DIAG_SIGNATURES.items()):
            if name in DIAG_SIGNATURES and os.environ.get("DEEQU_AMD_LIB") and not hasattr(l, name):
                continue  # (an older A/B build may lack a newer diagnostic export)
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(status: int):
    if status != DQ_OK:
        msg = lib().dq_last_error().decode("utf-8", "replace")
        if status == DQ_ERR_UNSUPPORTED:
            raise UnsupportedOnGpu(status, msg)
        raise DeequAmdError(status, msg)


def device_inputs(columns) -> bool:
    """True when one of `columns` (Columns, or None) is device-resident: its buffers are torch
    tensors in HBM that the library reads in place."""
    return any(getattr(c, "device", False) for c in columns)


# How a Plan orders a device batch with torch's current stream (A/B knob DEEQU_AMD_PLAN_ORDER; the
# measurements are in DESIGN.md, "Stream ordering at the Python boundary"):
#   "stream"            the plan's stream waits for the current one, then the current one for the scan
#   "host_then_stream"  the host waits for the current stream, then the current stream for the scan
PLAN_ORDER = "stream"


class StreamOrder:
    """The ordering of a library call after the work queued on torch's current stream of `device`
    ("Stream ordering at the Python boundary"): the library launches on streams of its own,
    which wait for no torch stream, so the kernel that writes an input -- or that still uses the memory
    of a freshly allocated output -- may not have run yet.  Used only for device-resident inputs or
    outputs (it imports torch), with the outputs allocated, right before the library call.

    `StreamOrder(device).wait()` (or `after_current_stream(device)`): the host waits for the current
    stream.  With `stream`, the hipStream_t every launch of an asynchronous call is ordered on, no host
    waits: `wait()` makes that stream wait for the current one (nothing at all when the current stream
    is idle) and returns it, and `release(current)` after the call makes the current stream wait for
    the call's kernels, so work queued there from then on may overwrite or free the call's inputs.  A
    handle keeps one StreamOrder: the torch stream and the event are made once, and `release` runs
    while the device already works on the call."""

    def __init__(self, device: int, stream: int = 0):
        self.device, self.stream = device, stream
        self._own = self._event = None
        self.mode = os.environ.get("DEEQU_AMD_PLAN_ORDER", PLAN_ORDER) if stream else "host"

    def wait(self):
        import torch
        current = torch.cuda.current_stream(self.device)
        if self.mode != "stream":
            current.synchronize()
            if self.mode == "host" or self._own is not None:
                return current
        if self._own is None:
            self._own = torch.cuda.ExternalStream(self.stream, device=torch.device("cuda", self.device))
            self._event = torch.cuda.Event()
        if self.mode == "stream" and not current.query():
            self._event.record(current)
            self._own.wait_event(self._event)
        return current

    def release(self, current) -> None:
        if self.mode == "stream" or self.mode == "host_then_stream":
            self._event.record(self._own)
            current.wait_event(self._event)


def after_current_stream(device: int) -> None:
    """The host waits for torch's current stream of `device` (StreamOrder)."""
    StreamOrder(device).wait()


PLAN_LAUNCHES = ("regex", "string_pass", "hll", "datatype", "strlen", "corr", "dec")


def diag_plan_groups(plan_handle):
    """dq_diag_plan_groups of a dq_plan: ([(kind, value type, np, tasks, blocks per task, resident
    workgroups per CU)] per scan group, {launch name: blocks per task, "rows", "dec_per_cu",
    "n_cu"}) of the plan's last consumed batch (tests assert the kernels and grids a plan ran)."""
    n = ctypes.c_int32(0)
    launches = (c_int64 * 10)()
    check(lib().dq_diag_plan_groups(plan_handle, None, 0, ctypes.byref(n), launches))
    groups = (c_int64 * (6 * max(1, n.value)))()
    check(lib().dq_diag_plan_groups(plan_handle, groups, n.value, ctypes.byref(n), launches))
    out = [tuple(groups[6 * g:6 * g + 6]) for g in range(n.value)]
    info = dict(zip(PLAN_LAUNCHES, launches[:7]))
    info.update(rows=launches[7], dec_per_cu=launches[8], n_cu=launches[9])
    return out, info


def diag_plan_lanemask(plan_handle):
    """dq_diag_plan_lanemask of a dq_plan: per scan task of the last consumed batch, True where
    the fast scan's lane-mask loop ran (False for tasks of the other kernels)."""
    n = ctypes.c_int32(0)
    check(lib().dq_diag_plan_lanemask(plan_handle, None, 0, ctypes.byref(n)))
    tasks = (c_int32 * max(1, n.value))()
    check(lib().dq_diag_plan_lanemask(plan_handle, tasks, n.value, ctypes.byref(n)))
    return [bool(tasks[t]) for t in range(n.value)]


REGEX_MODES = {"find_non_empty": 0, "find": 1, "full": 2}


def diag_regex_match(pattern: bytes, text: bytes, mode: str = "find_non_empty", want_image: bool = False):
    """dq_diag_regex_match_mode: (matched, DFA states, DFA columns[, the DFA image]) of the host
    build of the regex / LIKE compiler and walker in one of REGEX_MODES ("full": `pattern` is a SQL
    LIKE pattern).  Raises UnsupportedOnGpu with the compiler's message for a declined pattern."""
    m, ns, nc = c_int32(0), c_int32(0), c_int32(0)
    size = c_int64(0)
    args = (pattern, len(pattern), REGEX_MODES[mode], text, len(text), ctypes.byref(m), ctypes.byref(ns), ctypes.byref(nc))
    check(lib().dq_diag_regex_match_mode(*args, None, 0, ctypes.byref(size)))
    if not want_image:
        return m.value, ns.value, nc.value
    buf = ctypes.create_string_buffer(size.value)
    check(lib().dq_diag_regex_match_mode(*args, buf, size.value, ctypes.byref(size)))
    return m.value, ns.value, nc.value, buf.raw


def diag_plan_match_tasks(plan_handle):
    """(LIKE / RLIKE match tasks, distinct DFA images) of a dq_plan."""
    t, i = c_int32(0), c_int32(0)
    check(lib().dq_diag_plan_match_tasks(plan_handle, ctypes.byref(t), ctypes.byref(i)))
    return t.value, i.value


def diag_take_constants():
    """dq_diag_take_constants: {"rows_per_block", "scan_tile", "wave_bytes", "split_bytes"} of take's
    kernels (deequ_amd/csrc/dq_take.h)."""
    out = (c_int64 * 4)()
    check(lib().dq_diag_take_constants(out))
    return dict(zip(("rows_per_block", "scan_tile", "wave_bytes", "split_bytes"), out[:4]))


def device_count() -> int:
    n = c_int(0)
    check(lib().dq_device_count(ctypes.byref(n)))
    return n.value


class Context:
    """One dq_ctx per (process, device); created lazily."""

    _by_device = {}

    def __init__(self, device: int):
        self.device = device
        h = c_void_p()
        check(lib().dq_ctx_create(device, 0, ctypes.byref(h)))
        self.handle = h

    @classmethod
    def get(cls, device: int = 0) -> "Context":
        if device not in cls._by_device:
            cls._by_device[device] = Context(device)
        return cls._by_device[device]
