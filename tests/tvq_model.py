"""
A CPU model of the batched elementwise front end (csrc/svdq_ingest.hip; host layer ElementwiseBatch in ingest.py): what
a whole batch -- P ragged tensors x N tasks, flat lists parameter-major, index ``p * N + t`` -- has to produce, and the
inputs of the sweep in tests/test_hip_tvq_sweep.py.  numpy and the C oracle only: nothing from the package under test,
no torch ops, no GPU.  tests/test_tvq_model_cpu.py pins it to the vectors the reference produced (tests/golden/tvq.npz,
rtvq_cases.npz) and to the reference's formulas restated with torch CPU ops, and checks that the sweep's inputs can
tell a right kernel from a wrong one.

  ingest      fp32 ``finetuned - base``
  asymmetric  ``oracle.asym_quantize`` / ``asym_dequantize``: NaN-propagating min / max, scale = (1 / range) * qmax in
              two roundings, zero_point = -1 * rint(scale * min), code = clamp(rint(scale * x + zp), 0, qmax), a NaN
              code is 0; value = (q - zp) / scale
  absmax      scale of ``oracle.absmax_quantize`` ((1 / max|x|) * qmax, two roundings); code = rint(scale * x), 0 where
              that is NaN -- set here, not left to numpy's cast -- and clamped to [-128, 127] (int8) or
              [-32768, 32767] (int16, 16 bits) for the cast; value = q * scale
  add         fp32 ``add + value``, one rounding

Degenerate tensors have results too and the model defines them: a constant or all-zero tensor has range 0, scale = inf
and NaN values downstream; a NaN anywhere makes scale and zero point NaN and every code 0; +Inf makes the scale 0.

**The signed-zero rule.**  Everything is compared bit for bit (``helpers.bits_equal``: NaN equals NaN) with one
exception: where the expected ``zero_point`` is +-0 it is compared by value.  ``zero_point = -1 * rint(scale * min)``
carries the sign of a zero minimum, and when a tensor holds zeros of both signs which of them a reduction returns as the
minimum is an artefact of its order (torch returns +0.0 where the oracle returns -0.0; a wavefront's answer depends on
lane order).  Codes and dequantized values are the same bits either way: ``q - (+-0) == q``.  ``params_equal`` is that
rule.
"""
import warnings

import numpy as np

from helpers import bits_equal
from oracle import svd_hybrid_oracle as orc

ASYM_BITS = (1, 2, 3, 4, 5, 6, 7, 8)
ABSMAX_BITS = (2, 3, 4, 5, 6, 7, 8, 16)
WIDTHS = [("asymmetric", b) for b in ASYM_BITS] + [("absmax", b) for b in ABSMAX_BITS]

BLK_ROWS = 256                      # SVDQ_BLK_ROWS


# ------------------------------------------------------------------------------------------------ unit decomposition
def unit_rows(D, N):
    """``auto_unit_rows`` of csrc/svdq_api.hip: a function of the tensor's length and the task count alone."""
    ur = 8192 if N > 16 else 4096
    if D < 4 * ur:
        ur = -(-((D + 3) // 4) // BLK_ROWS) * BLK_ROWS
    return max(ur, 4 * BLK_ROWS)


def unit_lengths(D, N):
    """Lengths of the work units a D-element parameter of an N-task plan is cut into."""
    ur = unit_rows(D, N)
    return [min(ur, D - r0) for r0 in range(0, D, ur)]


# ------------------------------------------------------------------------------------------------ the operations
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def ingest(base, finetuned, N):
    """``base``: P arrays; ``finetuned``: P * N arrays.  Returns the P * N fp32 deltas."""
    assert len(finetuned) == len(base) * N
    with np.errstate(invalid="ignore", over="ignore"):
        return [_f32(finetuned[i]) - _f32(base[i // N]) for i in range(len(finetuned))]


def code_dtype(method, bits):
    return np.uint8 if method == "asymmetric" else (np.int16 if bits == 16 else np.int8)


def absmax_quantize(x, bits):
    xf = _f32(x)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)      # the oracle's own cast of a NaN product
        _, s = orc.absmax_quantize(xf, bits)
        r = np.rint((np.float32(s) * xf).astype(np.float32))
    lo, hi = (-32768.0, 32767.0) if bits == 16 else (-128.0, 127.0)
    r = np.clip(np.where(np.isnan(r), np.float32(0.0), r), lo, hi)
    return r.astype(code_dtype("absmax", bits)), np.float32(s)


def quantize(xs, bits, method):
    """Per tensor of ``xs``: (codes list, scale fp32 [len], zero_point fp32 [len] or None for absmax)."""
    codes, scale, zp = [], [], []
    for x in xs:
        if method == "asymmetric":
            q, s, z = orc.asym_quantize(_f32(x), bits)
            zp.append(z)
        else:
            q, s = absmax_quantize(x, bits)
        codes.append(q)
        scale.append(s)
    return codes, np.asarray(scale, dtype=np.float32), (np.asarray(zp, dtype=np.float32) if method == "asymmetric" else None)


def dequantize(codes, scale, zp, method, add=None, N=1):
    """Values of every tensor; ``add`` (P arrays, one per parameter) is added in fp32 when given."""
    out = []
    for i, q in enumerate(codes):
        with np.errstate(all="ignore"):
            if method == "asymmetric":
                v = orc.asym_dequantize(np.asarray(q).reshape(-1), scale[i], zp[i])
            else:
                v = orc.absmax_dequantize(np.asarray(q).reshape(-1), scale[i])
            if add is not None:
                v = _f32(add[i // N]) + v
        out.append(v.astype(np.float32))
    return out


def params_equal(got, want):
    """Zero points (or scales) against the model: bit for bit, by value where the expected one is +-0."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    if got.shape != want.shape:
        return False
    z = want == 0
    return bits_equal(got[~z], want[~z]) and bool(np.all(got[z] == 0))


# ------------------------------------------------------------------------------------------------ the sweep's inputs
RAMP = 511                          # elements of the ramp parameter: 2 * 255 + 1, a single unit with a 3-element tail
# one ragged list, short parameters behind long ones; the ramp is last
# 7940 = 3 * 2048 + 1796: 1796 itself is cut into 1024 + 772, so the unit of 1796 rows (a second unrolled trip for lane 0
# alone) needs a parameter of its own
SIZES = [4097, 1, 32771, 2, 768, 3, 16387, 4, 772, 5, 21508, 1020, 1023, 8188, 1027, 1796, 3073, 7940]
ROWS = SIZES + [RAMP]
RAMP_P = len(SIZES)
TASK_COUNTS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 20, 31, 32]
WIDTH_SWEEP_N = [1, 8, 9, 32]
ROUTE_WIDTHS = [("asymmetric", 4), ("absmax", 8)]
PLANTED_N = [3, 9, 20]
PLANTED_WIDTHS = [("asymmetric", 4), ("absmax", 8), ("absmax", 16)]
GRID_P = SIZES.index(768)           # this parameter's base lies on a 2^-8 grid: ``base + c`` and back is exact


def qmax_of(method, bits):
    return 2 ** bits - 1 if method == "asymmetric" else 2 ** (bits - 1) - 1


def ramp(method, bits, t=0):
    """Exact ties before the rounding at every width: asymmetric ``k / 2, k = 0 .. 2 qmax``; absmax ``+-k / 2`` with
    ``max |x| = qmax`` -- the scale is exactly 1 (times a power of two that moves with the task)."""
    q = qmax_of(method, bits)
    i = np.arange(RAMP)
    if method == "asymmetric":
        x = (i % (2 * q + 1)) / 2.0
    elif bits == 16:
        x = (i - 255) / 2.0
        x[0], x[-1] = -q, q
    else:
        x = (i % (4 * q + 1) - 2 * q) / 2.0
    return (x * 2.0 ** (t % 3 - 1)).astype(np.float32)


_random = {}


def _random_inputs(N):
    if N not in _random:
        rng = np.random.default_rng(20260 + N)
        base, ft = [], []
        for p, D in enumerate(SIZES):
            b = rng.standard_normal(D).astype(np.float32)
            if p == GRID_P:
                b = (np.rint(b * 256) / 256).astype(np.float32)
            base.append(b)
            for t in range(N):
                d = (0.01 * (1 + 0.25 * t) * rng.standard_normal(D)).astype(np.float32)
                d[int(rng.integers(D))] *= 3.0
                ft.append(b + d)
        for a in base + ft:
            a.setflags(write=False)
        _random[N] = (base, ft)
    return _random[N]


def slot(size, t, N):
    return SIZES.index(size) * N + t


def planted_slots(N):
    """{case: (size, task, ...)} of the non-finite and degenerate tensors ``sweep_inputs(planted=True)`` holds."""
    last = N - 1                    # the last task of a short group of k_ingest's eight-task walk (N = 3, 9, 20)
    return {"nan_vector": (4097, 1, 1300), "nan_tail": (3073, 0, 3072), "nan_tail2": (1027, last, 1026),
            "nan_last_task": (772, last, 5), "pinf": (1023, 0, 1021), "pinf_ninf": (1796, 1, 3, 1795),
            "constant": (768, 2), "zeros": (8188, 0), "zeros_short": (5, 1), "inf_minus_inf": (1020, 1, 7)}


def sweep_inputs(N, method="asymmetric", bits=8, planted=False):
    """(base: P arrays, finetuned: P * N arrays) of the sweep at N tasks: seeded random parameters of ``SIZES`` (task t's
    delta has its own spread and one outlier) and the ramp of (method, bits) over a zero base.  ``planted``: the slots of
    ``planted_slots`` hold NaN, +-Inf, a constant and all-zero deltas."""
    base, ft = _random_inputs(N)
    base, ft = list(base), list(ft)
    if planted:
        s = planted_slots(N)

        def edit(lst, i):
            lst[i] = lst[i].copy()
            return lst[i]
        for key in ("nan_vector", "nan_tail", "nan_tail2", "nan_last_task"):
            size, t, e = s[key]
            edit(ft, slot(size, t, N))[e] = np.nan
        size, t, e = s["pinf"]
        edit(ft, slot(size, t, N))[e] = np.inf
        size, t, e0, e1 = s["pinf_ninf"]
        x = edit(ft, slot(size, t, N))
        x[e0], x[e1] = np.inf, -np.inf
        size, t = s["constant"]
        ft[slot(size, t, N)] = base[SIZES.index(size)] + np.float32(0.375)
        for key in ("zeros", "zeros_short"):
            size, t = s[key]
            ft[slot(size, t, N)] = base[SIZES.index(size)].copy()
        size, t, e = s["inf_minus_inf"]      # base = finetuned = +Inf: NaN for this task, -Inf for the others
        edit(base, SIZES.index(size))[e] = np.inf
        edit(ft, slot(size, t, N))[e] = np.inf
    base.append(np.zeros(RAMP, dtype=np.float32))
    ft.extend(ramp(method, bits, t) for t in range(N))
    return base, ft


_expected = {}


def expected(N, method, bits, planted=False):
    """The model's results for ``sweep_inputs`` of the same arguments, shared by the cases that follow each other with the
    same arguments (the last four are kept): dict of ``base``, ``ft``,
    ``deltas``, ``codes``, ``scale``, ``zp``, ``values`` and ``values_add`` (``add`` = the base)."""
    key = (N, method, bits, planted)
    if key not in _expected:
        while len(_expected) >= 4:      # consecutive cases share a key; a whole sweep's results would be gigabytes
            _expected.pop(next(iter(_expected)))
        base, ft = sweep_inputs(N, method, bits, planted)
        deltas = ingest(base, ft, N)
        codes, scale, zp = quantize(deltas, bits, method)
        _expected[key] = {"base": base, "ft": ft, "deltas": deltas, "codes": codes, "scale": scale, "zp": zp,
                          "values": dequantize(codes, scale, zp, method),
                          "values_add": dequantize(codes, scale, zp, method, add=base, N=N)}
    return _expected[key]
