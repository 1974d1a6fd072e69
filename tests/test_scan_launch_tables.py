"""The universe test_gpu_scan_specialisations.py covers is the scan launch tables' (CPU only):
the kernels launch_values_np (dq_scan.hip) and fast_ptr / fast_kernel_for (dq_scan_fast.hip) name in
the source are exactly UNIVERSE plus UNREACHABLE, so a specialisation added to either table fails
here until the GPU coverage test knows it."""
import os
import re

import test_gpu_scan_specialisations as T
from scan_plans import CODE

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deequ_amd", "csrc")
C_TYPES = {"int8_t": "int8", "int16_t": "int16", "int32_t": "int32", "int64_t": "int64", "float": "float32",
           "double": "float64"}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_general_launch_table_is_the_universe():
    src = _src("dq_scan.hip")
    k_max = int(re.search(r"constexpr int kMaxPreds = (\d+);", _src("dq_internal.h")).group(1))
    body = src[src.index("static hipError_t launch_values_np"):src.index("hipError_t launch_scan_group")]
    nps = set()
    for np_, ext in re.findall(r"dq_scan_values_kernel<T, (\w+), (true|false)>", body):
        n = k_max if np_ == "kMaxPreds" else int(np_)
        nps.add(-1 if ext == "true" else n)
        assert ext == "false" or n == k_max
    group = src[src.index("hipError_t launch_scan_group"):src.index("int scan_group_blocks_per_cu")]
    types = {CODE[C_TYPES[t]] for t in re.findall(r"launch_values_np<(\w+)>", group)}
    assert len(types) == 6
    assert {(1, t, n) for t in types for n in nps} == {k for k in T.UNIVERSE if k[0] == 1}
    assert "dq_scan_bits_kernel" in group and (0, 0, 0) in T.UNIVERSE


def test_fast_launch_table_is_the_universe_and_the_unreachable():
    src = _src("dq_scan_fast.hip")
    pks = dict((name, int(v)) for name, v in re.findall(r"(PK_\w+) = (\d)", src[src.index("enum FastPK"):]))
    body = src[src.index("static const void* fast_ptr"):src.index("hipError_t launch_scan_fast")]
    named = {pks[p] for p in re.findall(r"dq_scan_fast_kernel<T, (PK_\w+), STATS, HLL>", body)}
    assert named == set(pks.values()) == {0, 1, 2, 3, 4}
    assert re.search(r"pk == PK_LT_I \|\| pk == PK_EQ_I\) return nullptr", body)  # fp64: no integer compares
    flags = {(s == "true", h == "true") for s, h in re.findall(r"fast_ptr<T, (true|false), (true|false)>", body)}
    assert len(flags) == 4
    want = set()
    for t, kinds in ((CODE["int64"], named), (CODE["float64"], named - {pks["PK_LT_I"], pks["PK_EQ_I"]})):
        want |= {(2, t, pk | (8 if s else 0) | (16 if h else 0)) for pk in kinds for s, h in flags}
    assert want == {k for k in T.UNIVERSE if k[0] == 2} | set(T.UNREACHABLE)
