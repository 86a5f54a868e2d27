"""
GPU sweep of the batched elementwise front end (csrc/svdq_ingest.hip: k_ingest<STATS>, k_tvq_stats, k_tvq_params,
k_tvq_apply, k_tvq_apply16, k_tvq_dequant, k_tvq_dequant16; host layer ingest.py) against the CPU model of
tests/tvq_model.py, which shares nothing with the kernels and is itself pinned to the reference's vectors and to torch
on the CPU (tests/test_tvq_model_cpu.py).

One ragged parameter list in one batch (``tvq_model.ROWS``: D < 4, units on both sides of the unrolled loops' bound, last
units that are only a scalar tail, a ramp with exact rounding ties), ``ElementwiseBatch``'s automatic unit size, every
task count of ``tvq_model.TASK_COUNTS``.  Deltas, codes, scales, zero points and dequantized values are compared bit for
bit (NaN equals NaN); the only exception is the signed-zero rule of the model's docstring for a zero point whose expected
value is +-0.  There is no tolerance in this file and no case is left out: constant, all-zero and non-finite tensors
have results the model defines.
"""
import numpy as np
import pytest
import torch

import tvq_model as tm
from helpers import bits_equal
from oracle import svd_hybrid_oracle as orc

pytestmark = pytest.mark.gpu

SENT = 0x5A
GAP = 64                    # sentinel bytes in front of and behind every carved output; offsets stay 16-byte aligned


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


@pytest.fixture(scope="module")
def dev(sq):
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ helpers
def _upload(arrays, dev):
    """The arrays as views of one device buffer, each at a 16-byte-aligned offset (one copy instead of hundreds)."""
    offs, n = [], 0
    for a in arrays:
        offs.append(n)
        n += (a.size + 3) & ~3
    flat = np.zeros(n, dtype=np.float32)
    for o, a in zip(offs, arrays):
        flat[o:o + a.size] = a
    buf = torch.from_numpy(flat).to(dev)
    views = [buf[o:o + a.size] for o, a in zip(offs, arrays)]
    assert all(v.data_ptr() % 16 == 0 for v in views)
    return views


def _table(tensors, dev):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(dev)


def _same(got, want, N, what):
    """A list of device tensors against the model's list: dtype, lengths and every bit."""
    assert len(got) == len(want), what
    assert [int(g.numel()) for g in got] == [w.size for w in want], what
    g = torch.cat([x.reshape(-1) for x in got]).cpu().numpy()
    w = np.concatenate([x.reshape(-1) for x in want])
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    equal = np.array_equal if w.dtype.kind in "iu" else bits_equal
    if equal(g, w):
        return
    o = 0
    for i, x in enumerate(want):
        seg = g[o:o + x.size]
        if not equal(seg, x.reshape(-1)):
            same = (seg.view(np.uint8).reshape(x.size, -1) == x.reshape(-1).view(np.uint8).reshape(x.size, -1)).all(axis=1)
            if w.dtype.kind == "f":
                same |= np.isnan(seg) & np.isnan(x.reshape(-1))
            bad = np.flatnonzero(~same)
            e = int(bad[0])
            raise AssertionError(f"{what}: parameter {i // N} (D = {x.size}), task {i % N}: {bad.size} elements differ, "
                                 f"first at {e}: got {seg[e]!r}, want {x.reshape(-1)[e]!r}")
        o += x.size
    raise AssertionError(what)


def _same_params(scale, zp, e, N, what):
    s = scale.cpu().numpy()
    bad = [i for i in range(s.size) if not bits_equal(s[i:i + 1], e["scale"][i:i + 1])]
    assert not bad, (what, "scale", [(i // N, i % N, s[i], e["scale"][i]) for i in bad[:4]])
    if e["zp"] is None:
        assert zp is None
        return
    z = zp.cpu().numpy()
    bad = [i for i in range(z.size) if not tm.params_equal(z[i:i + 1], e["zp"][i:i + 1])]
    assert not bad, (what, "zero point", [(i // N, i % N, z[i], e["zp"][i]) for i in bad[:4]])


def _run(sq, dev, N, method, bits, planted, stats_ready, through_ingest=True):
    """ingest -> quantize -> dequantize (plain, and fused with ``add`` = the base) of one batch, each stage against the
    model.  ``stats_ready``: the quantizer takes the statistics the ingest pass emitted instead of its own pass."""
    e = tm.expected(N, method, bits, planted)
    what = f"N={N} {method}{bits} planted={planted} stats_ready={stats_ready}"
    batch = sq.ElementwiseBatch(tm.ROWS, N, dev)
    try:
        base = _upload(e["base"], dev)
        if through_ingest:
            ft = _upload(e["ft"], dev)
            deltas = batch.ingest(base, ft, with_stats=stats_ready)
            _same(deltas, e["deltas"], N, what + ": deltas")
        else:
            assert not stats_ready
            deltas = _upload(e["deltas"], dev)
        codes, scale, zp = batch.quantize(deltas, bits, method, stats_ready=stats_ready)
        _same(codes, e["codes"], N, what + ": codes")
        _same_params(scale, zp, e, N, what)
        _same(batch.dequantize(codes, scale, zp, method), e["values"], N, what + ": values")
        _same(batch.dequantize(codes, scale, zp, method, add=base), e["values_add"], N, what + ": values + add")
        torch.cuda.synchronize()
    finally:
        batch.close()
    return e


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("N", tm.TASK_COUNTS)
def test_ingest(sq, dev, N, with_stats):
    e = tm.expected(N, "asymmetric", 8)
    batch = sq.ElementwiseBatch(tm.ROWS, N, dev)
    try:
        deltas = batch.ingest(_upload(e["base"], dev), _upload(e["ft"], dev), with_stats=with_stats)
        _same(deltas, e["deltas"], N, f"N={N} with_stats={with_stats}: deltas")
    finally:
        batch.close()


@pytest.mark.parametrize("stats_ready", [False, True])
@pytest.mark.parametrize("method,bits", tm.ROUTE_WIDTHS)
@pytest.mark.parametrize("N", tm.TASK_COUNTS)
def test_quantizer_routes(sq, dev, N, method, bits, stats_ready):
    """Each route against the model, not the routes against each other: the quantizer's own statistics pass, and the
    statistics ``ingest(with_stats=True)`` left behind."""
    _run(sq, dev, N, method, bits, planted=False, stats_ready=stats_ready)


@pytest.mark.parametrize("method,bits", tm.WIDTHS)
@pytest.mark.parametrize("N", tm.WIDTH_SWEEP_N)
def test_width_sweep(sq, dev, N, method, bits):
    """Asymmetric 1..8 bits, absmax 2..8 and 16 bits (int16 codes), dequantized with and without ``add``."""
    _run(sq, dev, N, method, bits, planted=False, stats_ready=False, through_ingest=False)


@pytest.mark.parametrize("stats_ready", [False, True])
@pytest.mark.parametrize("method,bits", tm.PLANTED_WIDTHS)
@pytest.mark.parametrize("N", tm.PLANTED_N)
def test_nonfinite_and_degenerate(sq, dev, N, method, bits, stats_ready):
    """NaN in a vector row, in the scalar tail and in the last task of a short group, +Inf, +Inf with -Inf, a constant,
    all zeros, and base = finetuned = +Inf, planted in chosen (parameter, task) slots: the model's scale, zero point,
    codes and values in those slots, and the slots next to them as if nothing had been planted."""
    e = _run(sq, dev, N, method, bits, planted=True, stats_ready=stats_ready)
    clean = tm.expected(N, method, bits, planted=False)
    s = tm.planted_slots(N)
    touched = {tm.slot(v[0], v[1], N) for v in s.values()} | {tm.slot(1020, u, N) for u in range(N)}
    for key in ("nan_vector", "nan_tail", "nan_tail2", "nan_last_task", "inf_minus_inf"):
        i = tm.slot(s[key][0], s[key][1], N)
        assert np.isnan(e["scale"][i]) and not e["codes"][i].any() and np.isnan(e["values"][i]).all(), key
    # _run held every slot to ``e``; the untouched ones of ``e`` are those of the clean batch
    for i in range(len(e["codes"])):
        if i not in touched:
            assert np.array_equal(e["codes"][i], clean["codes"][i]) and bits_equal(e["values"][i], clean["values"][i])


# ------------------------------------------------------------------------------------------------ nothing out of place
class Arena:
    """Outputs carved from one sentinel-filled allocation, ``GAP`` bytes between them, at 16-byte-aligned offsets."""

    def __init__(self, dev):
        self.dev, self.regions, self.size = dev, {}, GAP

    def reserve(self, name, nbytes):
        self.regions[name] = (self.size, int(nbytes))
        self.size += (int(nbytes) + 15) // 16 * 16 + GAP

    def allocate(self):
        self.buf = torch.full((self.size,), SENT, dtype=torch.uint8, device=self.dev)
        assert self.buf.data_ptr() % 16 == 0

    def view(self, name, dtype):
        o, n = self.regions[name]
        return self.buf[o:o + n].view(dtype)

    def check_gaps(self):
        host = self.buf.cpu().numpy()
        inside = np.zeros(self.size, dtype=bool)
        for o, n in self.regions.values():
            inside[o:o + n] = True
        wrong = np.flatnonzero(~inside & (host != SENT))
        assert wrong.size == 0, f"{wrong.size} bytes outside every output were written, first at offset {int(wrong[0])}"
        return host


def test_nothing_written_out_of_place(sq, dev):
    """Every kernel once straight through the C ABI as ingest.py calls it, N = 9 and the full size list, every output
    inside one sentinel-filled allocation: the outputs are the model's, the bytes between and behind them the sentinel."""
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import _ptr, _stream_ptr
    N = 9
    ea, ew = tm.expected(N, "asymmetric", 4), tm.expected(N, "absmax", 16)
    lib = nat.lib()
    batch = sq.ElementwiseBatch(tm.ROWS, N, dev)
    try:
        h = batch.plan._h
        assert int(batch.plan.sizes.n_units) == sum(len(tm.unit_lengths(D, N)) for D in tm.ROWS)
        work_bytes = int(lib.svdq_tvq_work_bytes(h))
        assert work_bytes >= int(batch.plan.sizes.n_units) * N * 16
        PN = len(tm.ROWS) * N
        ar = Arena(dev)
        kinds = (("plain", 4), ("stats", 4), ("c8", 1), ("v8", 4), ("c16", 2), ("v16", 4))
        for i in range(PN):
            for kind, item in kinds:
                ar.reserve(f"{kind}{i}", item * tm.ROWS[i // N])
        for name in ("scale_a", "zp_a", "scale_w"):
            ar.reserve(name, 4 * PN)
        ar.reserve("work", work_bytes)
        ar.allocate()
        dt = {"plain": torch.float32, "stats": torch.float32, "c8": torch.uint8, "v8": torch.float32,
              "c16": torch.int16, "v16": torch.float32}
        out = {kind: [ar.view(f"{kind}{i}", dt[kind]) for i in range(PN)] for kind, _ in kinds}
        assert all(v.data_ptr() % 16 == 0 for vs in out.values() for v in vs)
        scale_a, zp_a, scale_w = (ar.view(n, torch.float32) for n in ("scale_a", "zp_a", "scale_w"))
        work = ar.view("work", torch.uint8)
        base, ft = _upload(ea["base"], dev), _upload(ea["ft"], dev)
        base_w, x_w = _upload(ew["base"], dev), _upload(ew["deltas"], dev)
        tab = {k: _table(v, dev) for k, v in out.items()}
        tb, tf, tbw, txw = _table(base, dev), _table(ft, dev), _table(base_w, dev), _table(x_w, dev)
        st, null = _stream_ptr(), _ptr(None)
        nat.check(lib.svdq_ingest(h, _ptr(tb), _ptr(tf), _ptr(tab["plain"]), null, st), "svdq_ingest")
        nat.check(lib.svdq_ingest(h, _ptr(tb), _ptr(tf), _ptr(tab["stats"]), _ptr(work), st), "svdq_ingest")
        nat.check(lib.svdq_tvq_quantize(h, _ptr(tab["stats"]), 0, 4, _ptr(tab["c8"]), _ptr(scale_a), _ptr(zp_a),
                                        _ptr(work), 0, st), "svdq_tvq_quantize")
        nat.check(lib.svdq_tvq_dequantize(h, _ptr(tab["c8"]), 0, _ptr(scale_a), _ptr(zp_a), _ptr(tb), _ptr(tab["v8"]),
                                          st), "svdq_tvq_dequantize")
        nat.check(lib.svdq_tvq_quantize(h, _ptr(txw), 1, 16, _ptr(tab["c16"]), _ptr(scale_w), null, _ptr(work), 0, st),
                  "svdq_tvq_quantize")
        nat.check(lib.svdq_tvq_dequantize(h, _ptr(tab["c16"]), 2, _ptr(scale_w), null, _ptr(tbw), _ptr(tab["v16"]), st),
                  "svdq_tvq_dequantize")
        torch.cuda.synchronize()
        ar.check_gaps()
        _same(out["plain"], ea["deltas"], N, "k_ingest<false>")
        _same(out["stats"], ea["deltas"], N, "k_ingest<true>")
        _same(out["c8"], ea["codes"], N, "k_tvq_apply")
        _same_params(scale_a, zp_a, ea, N, "k_tvq_params asymmetric")
        _same(out["v8"], ea["values_add"], N, "k_tvq_dequant")
        _same(out["c16"], ew["codes"], N, "k_tvq_apply16")
        _same_params(scale_w, None, ew, N, "k_tvq_params absmax")
        _same(out["v16"], ew["values_add"], N, "k_tvq_dequant16")
    finally:
        batch.close()


# ------------------------------------------------------------------------------------------------ host layer
def test_ingest_state_dicts_33_tasks(sq, dev, capsys):
    """33 tasks chunk as 32 + 1; a parameter missing from two tasks and of another shape in a third forms a second
    group; a zero-element parameter; every task's vector against the oracle, in the base's key order."""
    rng = np.random.default_rng(33)
    shapes = {"a": (3, 5), "empty": (0, 4), "c": (6,), "b": (1,)}
    base = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}
    tasks = [f"t{t:02d}" for t in range(33)]
    fts = {}
    for j, t in enumerate(tasks):
        fts[t] = {k: (base[k] + 0.01 * (j + 1) * rng.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    del fts["t03"]["c"], fts["t17"]["c"]
    fts["t05"]["c"] = rng.standard_normal((2, 3)).astype(np.float32)
    got = sq.ingest_state_dicts({k: torch.from_numpy(v) for k, v in base.items()},
                                {t: {k: torch.from_numpy(v) for k, v in sd.items()} for t, sd in fts.items()}, device=dev)
    assert "Shape mismatch for c" in capsys.readouterr().out
    assert list(got.keys()) == tasks
    for t in tasks:
        want = orc.task_vector(base, fts[t])
        assert list(got[t].keys()) == list(want.keys()), t
        assert ("c" in want) == (t not in ("t03", "t05", "t17"))
        for k, w in want.items():
            v = got[t][k]
            assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == w.shape, (t, k)
            assert bits_equal(v.cpu().numpy(), w.astype(np.float32)), (t, k)


def _state(rng, shapes):
    return {k: (0.02 * rng.standard_normal(s) + 0.001).astype(np.float32) for k, s in shapes.items()}


def _check_payloads_and_values(sq, dev, state, bits_of, method, add_keys):
    """quantize_state_dict per width, the payloads mixed into one dictionary in the state's order, dequantize_payloads
    with ``add`` for ``add_keys`` only: payloads and values against the model."""
    rng = np.random.default_rng(5)
    payloads = {}
    for b in sorted(set(bits_of.values())):
        sub = {k: torch.from_numpy(v) for k, v in state.items() if bits_of[k] == b}
        part = sq.quantize_state_dict(sub, qbit=b, method=method, device=dev)
        assert list(part.keys()) == list(sub.keys())
        payloads.update(part)
    payloads = {k: payloads[k] for k in state}
    add = {k: rng.standard_normal(state[k].shape).astype(np.float32) for k in add_keys}
    model = {}
    for k, x in state.items():
        c, s, z = tm.quantize([x], bits_of[k], method)
        p = payloads[k]
        q = p["quantized"].cpu().numpy()
        assert q.dtype == tm.code_dtype(method, bits_of[k]) and q.shape == x.shape and tuple(p["shape"]) == x.shape, k
        assert np.array_equal(q.reshape(-1), c[0]), k
        assert p["scale"].dim() == 0 and bits_equal(p["scale"].cpu().numpy().reshape(1), s), k
        if method == "asymmetric":
            assert tm.params_equal(p["zero_point"].cpu().numpy(), z), k
        else:
            assert "zero_point" not in p
        model[k] = tm.dequantize(c, s, z, method, add=[add[k]] if k in add else None)[0]
    got = sq.dequantize_payloads(payloads, method=method, device=dev,
                                 add={k: torch.from_numpy(v) for k, v in add.items()})
    assert list(got.keys()) == list(state.keys())
    for k, v in got.items():
        assert tuple(v.shape) == state[k].shape and bits_equal(v.cpu().numpy().reshape(-1), model[k]), k
    return payloads


def test_mixed_int8_int16_payloads_with_partial_add(sq, dev):
    """int8 and int16 absmax payloads in one dictionary, ``add`` for one key of each kind and not for the others: all
    four launch groups of dequantize_payloads."""
    state = _state(np.random.default_rng(8), {"w0": (13, 79), "w1": (5,), "w2": (772,), "w3": (3, 100), "w4": (1,),
                                              "w5": (2049,)})
    bits_of = {"w0": 8, "w1": 16, "w2": 8, "w3": 16, "w4": 16, "w5": 5}
    pay = _check_payloads_and_values(sq, dev, state, bits_of, "absmax", add_keys=("w0", "w1", "w5"))
    kinds = {(k in ("w0", "w1", "w5"), pay[k]["quantized"].dtype == torch.int16) for k in state}
    assert len(kinds) == 4


def test_asymmetric_payloads_with_partial_add(sq, dev):
    state = _state(np.random.default_rng(9), {"w0": (13, 79), "w1": (5,), "w2": (772,), "w3": (3, 100), "w4": (2,)})
    bits_of = {"w0": 8, "w1": 3, "w2": 4, "w3": 1, "w4": 8}
    _check_payloads_and_values(sq, dev, state, bits_of, "asymmetric", add_keys=("w1", "w2"))


def test_misaligned_views_give_the_bits_of_their_aligned_copies(sq, dev):
    """``buf[1:1 + D]`` of a device tensor starts 4 bytes past a 16-byte boundary: the host layer clones it."""
    D = 1027
    rng = np.random.default_rng(12)
    bufs = [torch.from_numpy((0.02 * rng.standard_normal(D + 8)).astype(np.float32)).to(dev) for _ in range(3)]
    views = [b[o:o + D] for b, o in zip(bufs, (1, 2, 3))]
    assert all(v.data_ptr() % 16 != 0 for v in views)
    copies = [v.clone() for v in views]
    assert all(c.data_ptr() % 16 == 0 for c in copies)
    host = [c.cpu().numpy() for c in copies]
    for method, bits in (("asymmetric", 4), ("absmax", 8), ("absmax", 16)):
        a = sq.quantize_state_dict({"w": views[0]}, qbit=bits, method=method, device=dev)["w"]
        b = sq.quantize_state_dict({"w": copies[0]}, qbit=bits, method=method, device=dev)["w"]
        c, s, z = tm.quantize([host[0]], bits, method)
        for p in (a, b):
            assert np.array_equal(p["quantized"].cpu().numpy(), c[0])
            assert bits_equal(p["scale"].cpu().numpy().reshape(1), s)
            if z is not None:
                assert tm.params_equal(p["zero_point"].cpu().numpy(), z)
    got_v = sq.ingest_state_dicts({"w": views[0]}, {"t0": {"w": views[1]}, "t1": {"w": views[2]}}, device=dev)
    got_c = sq.ingest_state_dicts({"w": copies[0]}, {"t0": {"w": copies[1]}, "t1": {"w": copies[2]}}, device=dev)
    want = tm.ingest([host[0]], [host[1], host[2]], 2)
    for j, t in enumerate(("t0", "t1")):
        assert bits_equal(got_v[t]["w"].cpu().numpy(), want[j]) and bits_equal(got_c[t]["w"].cpu().numpy(), want[j])
