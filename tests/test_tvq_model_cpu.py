"""
tests/tvq_model.py without a GPU: the model against the vectors the reference produced (tests/golden/tvq.npz,
rtvq_cases.npz), against the reference's formulas restated here with torch CPU ops (quantization_utils.py:60-99, :134,
:172) on every edge input, and the conditions under which the sweep of tests/test_hip_tvq_sweep.py can tell a right
kernel from a wrong one -- conditions on the inputs, checked against the model alone.

Bit for bit throughout; the one exception is the signed-zero rule of the model's docstring (``params_equal``).
"""
import warnings

import numpy as np
import pytest
import torch

import tvq_model as tm
from helpers import bits_equal, load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("tvq.npz")


# ------------------------------------------------------------------------------------------------ reference vectors
def _check_payload(g, prefix, k, x, method, bits):
    codes, scale, zp = tm.quantize([x], bits, method)
    ref_q = g[f"{prefix}__q__{k}"]
    assert codes[0].dtype == ref_q.dtype and np.array_equal(codes[0], ref_q.reshape(-1)), (prefix, k)
    assert bits_equal(scale[0], g[f"{prefix}__scale__{k}"].astype(np.float32).reshape(())), (prefix, k)
    if method == "asymmetric":
        assert tm.params_equal(zp, g[f"{prefix}__zp__{k}"]), (prefix, k)
    else:
        assert f"{prefix}__zp__{k}" not in g
    return codes, scale, zp


@pytest.mark.parametrize("method", ["asymmetric", "absmax"])
def test_model_equals_reference_payloads(g, method):
    seen = 0
    for qbit in (8, 4, 3):
        prefix = f"qf__{method}{qbit}"
        for k in (str(x) for x in g[f"{prefix}__keys"]):
            c, s, z = _check_payload(g, prefix, k, g[f"ft__A__{k}"], method, qbit)
            want = g[f"{prefix}__deq__{k}"]
            assert bits_equal(tm.dequantize(c, s, z, method)[0].reshape(want.shape), want), (prefix, k)
            seen += 1
    # QuantizedBaseAndTaskVector: base at 8 bits, task vector at 4; dequantize() = base values + task values
    for k in (str(x) for x in g[f"qb__{method}__base__keys"]):
        cb, sb, zb = _check_payload(g, f"qb__{method}__base", k, g[f"base__{k}"], method, 8)
        ct, st, zt = _check_payload(g, f"qb__{method}__task", k, g[f"tv__A__{k}"], method, 4)
        vb = tm.dequantize(cb, sb, zb, method)
        want = g[f"qb__{method}__deq__{k}"]
        assert bits_equal(tm.dequantize(ct, st, zt, method, add=vb)[0].reshape(want.shape), want), k
        # QuantizedTaskVector over the same task payloads: its values, and base + values
        want = g[f"qt__{method}__deq__{k}"]
        assert bits_equal(tm.dequantize(ct, st, zt, method)[0].reshape(want.shape), want), k
        want = g[f"qt__{method}__applied__{k}"]
        assert bits_equal(tm.dequantize(ct, st, zt, method, add=[g[f"base__{k}"]])[0].reshape(want.shape), want), k
        seen += 1
    assert seen == 16                       # four parameters x (three widths + the base-and-task pair)
    assert sorted(g[f"qb__{method}__task__keys"].tolist()) == sorted(g[f"qb__{method}__base__keys"].tolist())


def test_model_equals_reference_task_vectors(g):
    keys = [str(k) for k in g["keys"]]
    for t in (str(x) for x in g["tasks"]):
        for k in (str(x) for x in g[f"tv_keys__{t}"]):
            got = tm.ingest([g[f"base__{k}"]], [g[f"ft__{t}__{k}"]], 1)[0]
            assert bits_equal(got, g[f"tv__{t}__{k}"].reshape(-1)), (t, k)
    assert "w1" in keys


def test_model_equals_rtvq_cases():
    r = load_golden("rtvq_cases.npz")
    names = sorted({k.split("__")[0] for k in r if "__asym8__q" in k})
    assert names
    for name in names:
        x = r[f"{name}__x"]
        for bits in (8, 4, 2):
            tag = f"{name}__asym{bits}__"
            c, s, z = tm.quantize([x], bits, "asymmetric")
            assert np.array_equal(c[0], r[tag + "q"].reshape(-1)), tag
            assert bits_equal(s[0], np.float32(r[tag + "scale"])) and tm.params_equal(z, r[tag + "zero_point"]), tag
            assert bits_equal(tm.dequantize(c, s, z, "asymmetric")[0], r[tag + "deq"].reshape(-1)), tag


# ------------------------------------------------------------------------------------------------ torch restatement
def _torch_asym(X, qbit):                   # quantization_utils.py:76-99
    X_min, X_max = X.min(), X.max()
    qmin, qmax = 0, 2 ** qbit - 1
    scale = (qmax - qmin) / (X_max - X_min)
    zero_point = -1 * torch.round(scale * X_min)
    X_q = torch.round(scale * X + zero_point).clamp(qmin, qmax)
    return X_q.to(torch.uint8), scale, zero_point


def _torch_absmax(X, qbit):                 # quantization_utils.py:60-73
    s = (2 ** (qbit - 1) - 1) / torch.max(torch.abs(X))
    X_q = (s * X).round()
    return X_q.to(torch.int8 if qbit <= 8 else torch.int16), s


def _edge_inputs():
    rng = np.random.default_rng(77)
    out = {}
    for n in (1, 2, 3, 4, 5, 7, 64, 255, 1023, 1024, 1027):
        out[f"random{n}"] = (0.02 * rng.standard_normal(n) + 0.003).astype(np.float32)
    for n in (1, 5, 1027):
        out[f"constant{n}"] = np.full(n, 0.375, dtype=np.float32)
        out[f"zeros{n}"] = np.zeros(n, dtype=np.float32)
    base = (0.02 * rng.standard_normal(1027)).astype(np.float32)
    for name, edits in (("nan", {300: np.nan}), ("pinf", {1025: np.inf}), ("pinf_ninf", {3: np.inf, 1026: -np.inf}),
                        ("huge", {0: 3e38, 1026: -3e38})):
        x = base.copy()
        for i, v in edits.items():
            x[i] = v
        out[name] = x
    out["nan1"] = np.array([np.nan], dtype=np.float32)
    out["pinf1"] = np.array([np.inf], dtype=np.float32)
    return out


@pytest.mark.parametrize("method,bits", tm.WIDTHS)
def test_model_equals_torch_restatement(method, bits):
    for name, x in _edge_inputs().items():
        X = torch.from_numpy(x.copy())
        c, s, z = tm.quantize([x], bits, method)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if method == "asymmetric":
                q_t, s_t, z_t = _torch_asym(X, bits)
                deq_t = (q_t.float() - z_t) / s_t                        # quantization_utils.py:172
                assert tm.params_equal(z, z_t.numpy().reshape(1)), (name, z, z_t)
            else:
                q_t, s_t = _torch_absmax(X, bits)
                deq_t = q_t.float() * s_t                                # quantization_utils.py:134
        assert c[0].dtype == q_t.numpy().dtype and np.array_equal(c[0], q_t.numpy()), (name, method, bits)
        assert bits_equal(s, s_t.numpy().reshape(1)), (name, s, s_t)
        assert bits_equal(tm.dequantize(c, s, z, method)[0], deq_t.numpy()), (name, method, bits)
        a = np.linspace(-1, 1, x.size, dtype=np.float32)
        assert bits_equal(tm.dequantize(c, s, z, method, add=[a])[0], (torch.from_numpy(a) + deq_t).numpy()), name


def test_signed_zero_minimum_is_the_only_freedom():
    """A minimum that is a zero present with both signs: the sign of zero_point follows the reduction's order; codes and
    values do not."""
    x = np.array([0.0, -0.0, 0.5, 1.0, -0.0, 0.0], dtype=np.float32)
    for bits in tm.ASYM_BITS:
        c, s, z = tm.quantize([x], bits, "asymmetric")
        q_t, s_t, z_t = _torch_asym(torch.from_numpy(x.copy()), bits)
        assert z[0] == 0 and float(z_t) == 0 and tm.params_equal(z_t.numpy().reshape(1), z)
        assert np.array_equal(c[0], q_t.numpy()) and bits_equal(s, s_t.numpy().reshape(1))
        assert bits_equal(tm.dequantize(c, s, z, "asymmetric")[0], ((q_t.float() - z_t) / s_t).numpy())
    assert tm.params_equal(np.float32([-0.0, 2.0]), np.float32([0.0, 2.0]))
    assert not tm.params_equal(np.float32([0.0, -2.0]), np.float32([0.0, 2.0]))
    assert not tm.params_equal(np.float32([1e-30, 2.0]), np.float32([0.0, 2.0]))
    assert tm.params_equal(np.float32([np.nan]), np.float32([np.nan]))


# ------------------------------------------------------------------------------------------------ the sweep can tell
def test_unit_decomposition_of_the_sweep_sizes():
    ul = tm.unit_lengths
    assert set(tm.SIZES) == {1, 2, 3, 4, 5, 768, 772, 1020, 1023, 1027, 1796, 3073, 4097, 7940, 8188, 16387, 21508, 32771}
    assert len(tm.SIZES) == 18 and tm.ROWS[-1] == tm.RAMP == 511
    assert sum(tm.ROWS) < 130000
    # a long parameter is followed by a short one
    assert any(a > 4096 and b < 4 for a, b in zip(tm.ROWS, tm.ROWS[1:]))
    for N in tm.TASK_COUNTS:
        for D in tm.ROWS:
            u = ul(D, N)
            assert sum(u) == D and all(0 < n <= tm.unit_rows(D, N) for n in u) and tm.unit_rows(D, N) % 256 == 0
        for D in (1, 2, 3, 4, 5, 768, 772, 1020, 1023, tm.RAMP):
            assert ul(D, N) == [D]
        # last units that are only a scalar tail
        assert ul(1027, N) == [1024, 3]
        assert ul(3073, N) == [1024, 1024, 1024, 1]
        assert ul(4097, N) == [1280, 1280, 1280, 257]
        assert ul(8188, N) == [2048, 2048, 2048, 2044]
        assert ul(1796, N) == [1024, 772]          # not a single unit: 7940 supplies the unit of 1796 rows
        assert ul(7940, N) == [2048, 2048, 2048, 1796]
        if N <= 16:
            assert ul(16387, N) == [4096] * 4 + [3]
            assert ul(21508, N) == [4096] * 5 + [1028]
            assert ul(32771, N) == [4096] * 8 + [3]
        else:
            assert ul(32771, N) == [8192] * 4 + [3]
            assert ul(16387, N)[-1] > 3 and len(ul(16387, N)) == 4
    # both sides of the unrolled loop's bound ``i + 768 < v1`` (i = 4 * lane at the unit's start), per unit: the number
    # of lanes that take an unrolled trip after k full ones
    def unrolled_lanes(n, last):
        v = n & ~3 if last else n
        return [sum(1 for lane in range(64) if 1024 * k + 4 * lane + 768 < v) for k in range(3)]
    assert unrolled_lanes(768, True) == [0, 0, 0]           # no lane
    assert unrolled_lanes(772, True) == [1, 0, 0]           # lane 0 alone
    assert unrolled_lanes(1020, True) == [63, 0, 0]         # all but the last lane
    assert unrolled_lanes(1023, True) == [63, 0, 0]
    assert unrolled_lanes(1024, False) == [64, 0, 0]
    assert unrolled_lanes(1028, True) == [64, 0, 0]         # one more row block for lane 0 in the plain loop
    assert unrolled_lanes(1796, True) == [64, 1, 0]
    assert unrolled_lanes(2044, True) == [64, 63, 0]
    assert unrolled_lanes(257, True) == [0, 0, 0]
    assert all(D < 4 for D in (1, 2, 3)) and {D & 3 for D in tm.ROWS} == {0, 1, 2, 3}


def _scale_two_roundings_differs(x, method, bits):
    q = np.float32(tm.qmax_of(method, bits))
    x = x[np.isfinite(x)]
    if x.size == 0:
        return False
    with np.errstate(all="ignore"):
        rng = np.float32(x.max()) - np.float32(x.min()) if method == "asymmetric" else np.float32(np.abs(x).max())
        if not np.isfinite(rng) or rng == 0:
            return False
        two = np.float32(np.float32(1.0) / rng) * q
        one = q / rng
    return two != one


def _sweep_cases():
    for N in tm.TASK_COUNTS:
        for method, bits in (tm.WIDTHS if N in tm.WIDTH_SWEEP_N else tm.ROUTE_WIDTHS):
            yield N, method, bits


def test_sweep_has_two_rounding_scales_at_every_width():
    """(1 / range) * qmax in two roundings against qmax / range in one: a kernel that divides once is caught only by a
    tensor where the two differ.  Every case of the sweep holds one (1 bit, qmax = 1, cannot)."""
    assert np.float32(np.float32(1.0) / np.float32(3.0)) * np.float32(3.0) == np.float32(1.0)      # why not all do
    for N, method, bits in _sweep_cases():
        if tm.qmax_of(method, bits) == 1:
            continue
        e = tm.expected(N, method, bits)
        hits = sum(_scale_two_roundings_differs(d, method, bits) for d in e["deltas"])
        assert hits >= 1, (N, method, bits)
        # and the model took the two-rounding one
        for i, d in enumerate(e["deltas"]):
            if _scale_two_roundings_differs(d, method, bits):
                rng = d.max() - d.min() if method == "asymmetric" else np.abs(d).max()
                assert e["scale"][i] != np.float32(tm.qmax_of(method, bits)) / np.float32(rng)
                break


def _half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))


@pytest.mark.parametrize("method,bits", tm.WIDTHS)
def test_ramp_has_exact_ties(method, bits):
    """Half-to-even (rintf) and half-away (roundf) give different codes on the ramp at every width."""
    qm = np.float32(tm.qmax_of(method, bits))
    assert np.float32(np.float32(1.0) / qm) * qm == np.float32(1.0)
    for t in range(3):
        x = tm.ramp(method, bits, t)
        assert x.size == tm.RAMP and x.dtype == np.float32
        c, s, z = tm.quantize([x], bits, method)
        assert s[0] == np.float32(2.0 ** -(t % 3 - 1))                 # exactly 1, times the task's power of two
        v = s[0] * x if method == "absmax" else s[0] * x + z[0]
        ties = np.abs(v - np.trunc(v)) == 0.5
        assert ties.sum() >= 2 and np.all(v * 2 == np.rint(v * 2))
        lo, hi = (0, qm) if method == "asymmetric" else ((-32768, 32767) if bits == 16 else (-128, 127))
        away = np.clip(_half_away(v), lo, hi).astype(c[0].dtype)
        assert not np.array_equal(away, c[0]), (method, bits, t)
        if method == "asymmetric":
            assert c[0].min() == 0 and c[0].max() == qm
        else:
            assert c[0].min() == -qm and c[0].max() == qm
    # the sweep's ramp parameter is this ramp, through ingest over a zero base
    e = tm.expected(3, method, bits)
    for t in range(3):
        assert bits_equal(e["deltas"][tm.RAMP_P * 3 + t], tm.ramp(method, bits, t))


def test_int16_codes_leave_the_int8_range():
    for N in tm.WIDTH_SWEEP_N:
        e = tm.expected(N, "absmax", 16)
        assert all(np.abs(c.astype(np.int32)).max() > 127 for c, d in zip(e["codes"], e["deltas"]) if d.size > 1)
        assert all(c.dtype == np.int16 for c in e["codes"])


@pytest.mark.parametrize("N", tm.PLANTED_N)
def test_planted_slots_hold_what_they_claim(N):
    s = tm.planted_slots(N)
    clean = tm.expected(N, "asymmetric", 4)
    clean = {"deltas": clean["deltas"], "scale": clean["scale"]}
    e = tm.expected(N, "asymmetric", 4, planted=True)
    d = e["deltas"]

    def D(key):
        return d[tm.slot(s[key][0], s[key][1], N)]
    assert N - 1 >= 2 and (N - 1) % 8 in (0, 2, 3) and N % 8 != 0          # the last task sits in a short group
    for key in ("nan_vector", "nan_tail", "nan_tail2", "nan_last_task", "inf_minus_inf"):
        x = D(key)
        assert np.isnan(x).sum() == 1 and np.isnan(x[s[key][2]]), key
        i = tm.slot(s[key][0], s[key][1], N)
        assert np.isnan(e["scale"][i]) and np.isnan(e["zp"][i]) and not e["codes"][i].any(), key
    size, t, el = s["nan_vector"]
    assert el < (size & ~3) and el % 256 // 4 != 0                           # a vector row, not lane 0's
    for key in ("nan_tail", "nan_tail2"):
        size, t, el = s[key]
        assert el >= (size & ~3) and tm.unit_lengths(size, N)[-1] < 4        # in a unit that is only a scalar tail
    assert s["nan_tail2"][2] - (1027 & ~3) == 2                              # not lane 0
    assert np.isposinf(D("pinf")).sum() == 1 and not np.isneginf(D("pinf")).any()
    assert np.isposinf(D("pinf_ninf")).sum() == 1 and np.isneginf(D("pinf_ninf")).sum() == 1
    assert e["scale"][tm.slot(1023, 0, N)] == 0 and np.isnan(e["zp"][tm.slot(1796, 1, N)])
    c = D("constant")
    assert c.size == 768 and np.all(c == np.float32(0.375))
    assert np.isinf(e["scale"][tm.slot(768, 2, N)])
    for key in ("zeros", "zeros_short"):
        z = D(key)
        assert not z.any() and not np.signbit(z).any() and np.isinf(e["scale"][tm.slot(s[key][0], s[key][1], N)])
    # base = finetuned = +Inf: NaN for that task, -Inf for every other task of the parameter
    size, t, el = s["inf_minus_inf"]
    for u in range(N):
        x = d[tm.slot(size, u, N)][el]
        assert np.isnan(x) if u == t else np.isneginf(x)
    # every other slot is what it was without the planting: a NaN must not reach its neighbours
    touched = {tm.slot(v[0], v[1], N) for v in s.values()} | {tm.slot(1020, u, N) for u in range(N)}
    for i in range(len(d)):
        if i not in touched:
            assert bits_equal(d[i], clean["deltas"][i]) and bits_equal(e["scale"][i:i + 1], clean["scale"][i:i + 1])
            assert np.isfinite(e["scale"][i]) or d[i].size == 1
    for v in s.values():                      # each planted slot has untouched neighbours in its parameter
        assert any(tm.slot(v[0], u, N) not in touched for u in range(N)) or v[0] == 1020
