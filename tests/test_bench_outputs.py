"""bench.py's command line and `--dump-outputs` arrays, on the host: `--full` exists and is off
by default; a dq_state array becomes float64 arrays that hold every field exactly (the 64-bit HLL
register words as two 32-bit halves); the GPU run is in test_gpu_bench_plain.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from deequ_amd import _lib as L  # noqa: E402


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_full_and_dump_outputs_options(monkeypatch):
    plain = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert plain.full is False and plain.dump_outputs is None and (plain.steps, plain.warmup) == (7, 2)
    full = _args(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert full.full is True and full.dump_outputs == "somewhere"


def test_help_renders(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--help"])
    try:
        bench.parse_args()
    except SystemExit as e:
        assert e.code == 0
    out = capsys.readouterr().out
    assert "--full" in out and "--dump-outputs" in out


def test_states_arrays_hold_every_field_exactly(tmp_path):
    raw = (L.DqState * 3)()
    raw[0].kind, raw[0].has_value, raw[0].num_matches = 1, 1, 1_000_000_000
    raw[1].kind, raw[1].has_value, raw[1].count, raw[1].sum = 4, 1, 949_999_999, -1.25e18
    raw[1].n, raw[1].avg, raw[1].m2, raw[1].value = 9.5e8, 1e3 + 2 ** -40, 9.5e12, float("-inf")
    raw[2].y_avg, raw[2].ck, raw[2].x_mk, raw[2].y_mk = 1.5, -2.5, 3.5, 4.5
    words = [-1, -2 ** 63, 2 ** 63 - 1, 0x0123456789ABCDEF, 0] + list(range(5, L.DQ_HLL_NUM_WORDS))
    for k, w in enumerate(words):
        raw[2].words[k] = w
    a = bench._states_arrays(raw, 3)
    s, h = a["states"], a["hll_words"]
    assert s.dtype == np.float64 and h.dtype == np.float64
    assert s.shape == (3, len(bench._STATE_FIELDS)) and h.shape == (3, 2 * L.DQ_HLL_NUM_WORDS)
    for i in range(3):
        for j, f in enumerate(bench._STATE_FIELDS):
            assert s[i, j] == float(getattr(raw[i], f)), (i, f)
    lo, hi = h[2, :L.DQ_HLL_NUM_WORDS], h[2, L.DQ_HLL_NUM_WORDS:]
    back = [(int(x) | (int(y) << 32)) for x, y in zip(lo, hi)]
    assert back == [w % 2 ** 64 for w in words]
    assert not h[:2].any()

    class A:
        dump_outputs = str(tmp_path / "out")
    bench._dump_outputs(A, 1, a)  # only rank 0 writes
    assert not os.path.exists(A.dump_outputs)
    bench._dump_outputs(A, 0, a)
    assert sorted(os.listdir(A.dump_outputs)) == ["hll_words.npy", "states.npy"]
    assert np.array_equal(np.load(os.path.join(A.dump_outputs, "states.npy")), s)
    assert np.load(os.path.join(A.dump_outputs, "hll_words.npy")).dtype == np.float64
