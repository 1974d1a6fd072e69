"""Device inputs whose producer is still queued on torch's current stream when the library is called.

`Table.to_device()` copies from pageable memory and has finished when it returns, so a test built
on it never calls the library while the kernel that writes its input is still running.  Here the
input tensors are uploaded holding a SENTINEL content; the REAL content sits in a second set of
tensors; `delayed` queues a calibrated `torch.cuda._sleep` and then `dst.copy_(real)` on the current
stream and returns an event recorded behind the copies.  An entry point that orders itself after
the current stream ("Stream ordering at the Python boundary") computes the real data's
result; one that does not reads the sentinel, whose result differs.

Memory safety is part of the design: a premature or interleaved read must give a wrong answer, never
an out-of-range access.  Real and sentinel columns have identical string offsets (fixed 4-byte
strings, uploaded ready-made), sentinel row indices are valid row numbers, decimal words keep a zero
high word, and every byte-wise mix of the two contents is a valid input.

Shapes: N = 20 001 rows (no multiple of 64, several blocks); 5 % NULL in the real data, none in the
sentinel (both carry a validity bitmap, so the buffers have one shape)."""
from collections import OrderedDict

import numpy as np

import deequ_amd as d

N = 20_001
WIDTH = 4               # bytes of every string
DEFAULT_MS = 150.0      # the delay, unless a call needs a longer one (20x its own duration)
MAX_MS = 500.0          # never longer: nothing may look like a hang
DECIMAL = "decimal(10,2)"

_CYCLES_PER_MS = {}


def calibrated_sleep(dev, ms=DEFAULT_MS):
    """Queues a `torch.cuda._sleep` of about `ms` milliseconds on the current stream of `dev`.  The
    cycle count comes from one timed `_sleep` per process (between two events)."""
    import torch
    if not 0 < ms <= MAX_MS:
        raise ValueError("a delay of %r ms: at most %d" % (ms, MAX_MS))
    dev = torch.device(dev)
    if dev.index not in _CYCLES_PER_MS:
        c0 = 2_000_000
        torch.cuda._sleep(c0)  # (loads the kernel)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(c0)
        e1.record()
        e1.synchronize()
        _CYCLES_PER_MS[dev.index] = c0 / e0.elapsed_time(e1)
    cycles = int(_CYCLES_PER_MS[dev.index] * ms)
    torch.cuda._sleep(cycles)
    return cycles


def measured_sleep_ms(dev, ms=DEFAULT_MS):
    """How long `calibrated_sleep(dev, ms)` lasts on the device."""
    import torch
    calibrated_sleep(dev, 1.0)  # (calibrates outside the timed span)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    calibrated_sleep(dev, ms)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def upload(arrays, dev="cuda:0"):
    """Host arrays (None stays None) as device tensors, complete on return."""
    import torch
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:  # (a decimal column's words travel as int64 bits)
            a = a.view(np.int64)
        out.append(torch.from_numpy(a).to(dev))
    torch.cuda.synchronize(dev)
    return out


def delayed(real_tensors, sentinel_tensors, ms=DEFAULT_MS):
    """`sentinel_tensors` are the destinations: device tensors that hold the sentinel content now.
    Queues, on the current stream, the calibrated sleep and then `dst.copy_(real)` for every pair,
    and returns an event recorded behind the copies.  The caller asserts `not ev.query()` on the
    line before the library call: a delay that has run out by then is a failure, not a pass."""
    import torch
    pairs = [(t, r) for t, r in zip(sentinel_tensors, real_tensors) if t is not None]
    for t, r in pairs:
        assert t.shape == r.shape and t.dtype == r.dtype and t.device == r.device
    calibrated_sleep(pairs[0][0].device, ms)
    for t, r in pairs:
        t.copy_(r)
    ev = torch.cuda.Event()
    ev.record()
    return ev


def _buffers(col):
    return [col.values, col.validity, col.offsets]


def device_table(host, buffers):
    """A device-resident Table with the layout of the host Table `host` over `buffers`, three per
    column (values, validity, offsets) in column order."""
    cols = OrderedDict()
    for i, (name, c) in enumerate(host.columns.items()):
        v, b, o = buffers[3 * i:3 * i + 3]
        cols[name] = d.Column(c.dtype, c.length, v, b, o, c.offset, device=True)
    return d.Table(cols)


def delayed_table(real, sentinel, ms=DEFAULT_MS):
    """(a device Table that holds `sentinel` until the delayed copies of `real` land, their event)."""
    assert list(real.schema.items()) == list(sentinel.schema.items())
    dst = upload([b for c in sentinel.columns.values() for b in _buffers(c)])
    src = upload([b for c in real.columns.values() for b in _buffers(c)])
    return device_table(sentinel, dst), delayed(src, dst, ms)


def synced_table(host):
    """`host` in HBM, complete on return (what the rest of the suite tests)."""
    return device_table(host, upload([b for c in host.columns.values() for b in _buffers(c)]))


# ---------------------------------------------------------------- the two contents
def _validity(rng, n, null_frac):
    valid = rng.random(n) >= null_frac if null_frac else np.ones(n, dtype=bool)
    return np.packbits(valid, bitorder="little")


def _strings(codes, alphabet):
    """Fixed-width strings: `codes` is an (n, WIDTH) array of indices into `alphabet`."""
    heap = np.frombuffer(alphabet, dtype=np.uint8)[codes].reshape(-1)
    return np.concatenate([heap, np.zeros(8, np.uint8)])  # (8 spare bytes, as Column.from_pylist leaves)


OFFSETS = (np.arange(N + 1, dtype=np.int64) * WIDTH).astype(np.int32)
_DIGITS, _LETTERS = b"0123456789", b"abcdefghijklmnopqrstuvwxyz"


def _content(sentinel: bool):
    """Every column of the harness with the real or the sentinel content:
    i int64, f and g float64, b bool, s 4-digit strings (letters in the sentinel), k a few-valued
    string (40 values), x strings like "12.5" (letters in the sentinel), id a unique int64 key,
    dec a decimal(10,2) of non-negative values."""
    rng = np.random.default_rng(2 if sentinel else 1)
    nf = 0.0 if sentinel else 0.05
    cols = OrderedDict()

    def add(name, dtype, values, offsets=None):
        cols[name] = d.Column(dtype, N, values, _validity(rng, N, nf), offsets)

    add("i", "int64", rng.integers(5000, 6000, N) if sentinel else rng.integers(-1000, 1000, N))
    f = rng.normal(-5e3, 1e2, N) if sentinel else rng.normal(1e3, 1e2, N)
    add("f", "float64", f)
    add("g", "float64", rng.random(N) if sentinel else 0.5 * f + rng.normal(0.0, 30.0, N))
    add("b", "bool", np.packbits(rng.random(N) < (0.9 if sentinel else 0.3), bitorder="little"))
    add("s", "string", _strings(rng.integers(0, 26 if sentinel else 10, (N, WIDTH)), _LETTERS if sentinel else _DIGITS),
        OFFSETS)
    few = rng.integers(0, 40, N)
    codes = np.stack([np.zeros(N, np.int64), np.zeros(N, np.int64), few // 10, few % 10], axis=1)
    add("k", "string", _strings(codes + (5 if sentinel else 0), _LETTERS if sentinel else _DIGITS), OFFSETS)
    if sentinel:
        x = _strings(rng.integers(0, 26, (N, WIDTH)), _LETTERS)
    else:
        num = rng.integers(0, 1000, N)
        x = _strings(np.stack([num // 100, num // 10 % 10, np.full(N, 10), num % 10], axis=1), _DIGITS + b".")
    add("x", "string", x, OFFSETS)
    add("id", "int64", rng.permutation(N).astype(np.int64) + (N if sentinel else 0))
    words = np.zeros((N, 2), dtype=np.uint64)
    words[:, 0] = rng.integers(10 ** 8, 10 ** 9, N) if sentinel else rng.integers(0, 10 ** 6, N)
    add("dec", DECIMAL, words)
    return cols


_CONTENT = {}


def tables(*names):
    """(real, sentinel): host Tables of the columns `names`, same layout, different content."""
    for sentinel in (False, True):
        if sentinel not in _CONTENT:
            _CONTENT[sentinel] = _content(sentinel)
    return tuple(d.Table(OrderedDict((n, _CONTENT[s][n]) for n in names)) for s in (False, True))


# ---------------------------------------------------------------- comparing results
def same(a, b, rtol=1e-9):
    """Structural equality of two results of one API over the same data.  Floating-point values
    compare within `rtol`: two runs of a reduction may add their partial sums in another order, which
    moves a sum of 2e4 terms by a few 1e-12 of its magnitude; the sentinel's results differ in their
    leading digits."""
    if isinstance(a, dict):  # (in any order: a frequency table lists its groups in slot order)
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(v, b[k], rtol) for k, v in a.items())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y, rtol) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.dtype.kind == "f":
            return bool(np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True))
        return bool(np.array_equal(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and (a == b or (a != a and b != b) or abs(a - b) <= rtol * max(abs(a), abs(b)))
    if isinstance(a, d.State) and type(a) is type(b) and \
            all(isinstance(v, (int, float)) for v in list(vars(a).values()) + list(vars(b).values())):
        return same(vars(a), vars(b), rtol)
    return bool(a == b)


def differences(a, b, path="result", limit=6):
    """Where two results differ, for an assertion's message: at most `limit` lines "path: a != b"."""
    out = []

    def walk(x, y, p):
        if len(out) >= limit or same(x, y):
            return
        if isinstance(x, dict) and isinstance(y, dict) and x.keys() == y.keys():
            for k in x:
                walk(x[k], y[k], "%s[%s]" % (p, k))
        elif isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)) and len(x) == len(y):
            for i, (u, v) in enumerate(zip(x, y)):
                walk(u, v, "%s[%d]" % (p, i))
        elif isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.shape == y.shape and x.dtype == y.dtype:
            at = np.flatnonzero(x.reshape(-1) != y.reshape(-1))
            out.append("%s: %d of %d elements differ, first at %s" % (p, at.size, x.size, at[:4].tolist()))
        else:
            out.append("%s: %.200r != %.200r" % (p, x, y))
    walk(a, b, path)
    return "\n".join(out)


def host_column(col):
    """The buffers of a device Column as host arrays (values, validity, offsets; a string heap up
    to its last offset)."""
    def down(t):
        return None if t is None else t.cpu().numpy()
    values, offsets = down(col.values), down(col.offsets)
    if offsets is not None:
        values = values[:int(offsets[-1])]
    return (col.dtype, col.length, values, down(col.validity), offsets)


def snapshot(table):
    """Clones every buffer of a device Table with torch ops on the current stream, right now: what a
    caller's next kernel would read (no device-wide wait in between)."""
    cols = OrderedDict()
    for name, c in table.columns.items():
        v, b, o = (None if t is None else t.clone() for t in _buffers(c))
        cols[name] = d.Column(c.dtype, c.length, v, b, o, c.offset, device=True)
    return d.Table(cols)


def host_table(table):
    return {name: host_column(c) for name, c in table.columns.items()}
