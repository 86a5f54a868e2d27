"""
GPU tests of the diagnostics straight from checkpoints (svdq_diagnostics_from_base / _masked_from_base: k_diag's
minus-base mode, include/svdq.h): the fine-tuned and the base tensors go in, ``finetuned - base`` is formed inside the
pass.  The contract is on bits -- the result is what svdq_diagnostics / svdq_diagnostics_masked give on fp32 tensors
holding ``ft.float() - base.float()`` -- so the comparisons against the materialised deltas have no tolerance; the
truth of the numbers is held to the fp64 formula at the bar of tests/test_hip_diagnostics.py (helpers.diag_check).

Inputs: low-rank deltas with spikes at block boundaries (as tests/test_hip_diagnostics.py), a seeded O(1) ``base`` and
``ft = base + delta`` stored in the test's dtype, so that the subtraction really rounds.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import diag_check

pytestmark = pytest.mark.gpu

SIZES = [9000, 257, 4096 * 3 + 5, 1, 8192 + 300, 13, 40, 17]      # short last tiles after long parameters, blocks < RB
MSIZES = [9000, 300, 4096 * 3 + 5, 8192 + 300, 61, 150]
MDENS = [0.9, 0.5, 0.97, 0.15, 0.3, 0.8]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _dev():
    return torch.device("cuda", 0)


def _spiked(vecs, sizes):
    """One large element per task at a block / unit boundary row: a row that a kernel drops or counts twice cannot hide."""
    for p, D in enumerate(sizes):
        spots = [s for s in (0, 63, 64, 127, 128, 255, 256, 4095, 4096, 8191, 8192, D - 2, D - 1) if 0 <= s < D]
        for t, v in enumerate(vecs[p]):
            v[spots[(t + p) % len(spots)]] += 3.0 + 0.25 * t
    return vecs


def _table(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(_dev())


def _checkpoints(sizes, n, dtype, seed0):
    """(ft [P][N] of ``dtype``, base [P] of ``dtype``, delta [P][N] fp32 = ft.float() - base.float()), on the device."""
    from oracle import svd_hybrid_oracle as orc
    dev = _dev()
    gen = torch.Generator().manual_seed(seed0 + n)
    vecs = _spiked([[d.clone() for d in orc.synthetic_deltas(D, n, seed0 + i, rank=3)] for i, D in enumerate(sizes)], sizes)
    base = [torch.randn(D, generator=gen).to(dtype).to(dev) for D in sizes]
    ft = [[(b.float() + d.to(dev)).to(dtype) for d in vs] for b, vs in zip(base, vecs)]
    delta = [[f.float() - b.float() for f in fs] for b, fs in zip(base, ft)]
    return ft, base, delta


def _same(a, b):
    """Element for element on the doubles, NaN at the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def _plan(sq, sizes, n, fp16, center, dtype=torch.float32, max_rank=None):
    from svdq_amd.pipeline import CompressPlan
    return CompressPlan(sizes, n, energy_threshold=0.9, max_rank=max_rank, center=center, fp16=fp16, low_bits=4,
                        rtvq_stages=2, device=_dev(), input_dtype=dtype)


_PLAIN = {}


def _plain(sq, n, fp16, center, max_rank=None):
    """One compressed plan per variant, shared by the tests below: (plan, ft, base, delta, ft table, base table,
    result of diagnostics_from_base, result of diagnostics on the materialised deltas)."""
    key = (n, fp16, center, max_rank)
    if key not in _PLAIN:
        ft, base, delta = _checkpoints(SIZES, n, torch.float32, 300)
        plan = _plan(sq, SIZES, n, fp16, center, max_rank=max_rank)
        ftab, btab = plan.pointer_table(ft), _table(base)
        plan.run_from_base(ftab, btab)
        plan.fetch_small()
        got = plan.diagnostics_from_base(ftab, btab).cpu().numpy()
        want = plan.diagnostics(_table([d for ds in delta for d in ds])).cpu().numpy()
        _PLAIN[key] = (plan, ft, base, delta, ftab, btab, got, want)
    return _PLAIN[key]


# ------------------------------------------------------------------------------------------ 1. bits, plain
@pytest.mark.parametrize("n_tasks", [3, 4, 8, 12, 20, 32])
@pytest.mark.parametrize("fp16,center", [(True, True), (True, False), (False, True), (False, False)])
def test_from_base_is_bit_for_bit_the_materialised_deltas(sq, n_tasks, fp16, center):
    plan, ft, base, delta, ftab, btab, got, want = _plain(sq, n_tasks, fp16, center)
    assert got.shape == (len(SIZES), n_tasks, 6)
    assert _same(got, want)
    assert np.isfinite(want).any()
    dtab = _table([d for ds in delta for d in ds])
    if center:
        assert _same(plan.diagnostics_from_base(ftab, btab, add_mean=True).cpu().numpy(),
                     plan.diagnostics(dtab, add_mean=True).cpu().numpy())


# ------------------------------------------------------------------------------------------ 2. bits, half inputs
@pytest.mark.parametrize("n_tasks", [8, 20])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_checkpoints_give_the_fp32_plan_bits(sq, n_tasks, dtype):
    ft, base, delta = _checkpoints(SIZES, n_tasks, dtype, 340)
    H = _plan(sq, SIZES, n_tasks, True, True, dtype)
    F = _plan(sq, SIZES, n_tasks, True, True)
    ftab, btab = H.pointer_table(ft), _table(base)
    H.run_from_base(ftab, btab)
    dtab = F.pointer_table(delta)
    F.run(dtab)
    torch.cuda.synchronize()
    assert torch.equal(H.small, F.small)
    assert _same(H.diagnostics_from_base(ftab, btab).cpu().numpy(), F.diagnostics(dtab).cpu().numpy())
    assert _same(H.diagnostics_from_base(ftab, btab, add_mean=True).cpu().numpy(),
                 F.diagnostics(dtab, add_mean=True).cpu().numpy())
    H.close(), F.close()


# ------------------------------------------------------------------------------------------ 3. bits, masked
_MASKED = {}


def _masked(sq, n, fp16, inverted, center=False, max_rank=None):
    """Set up as tests/test_hip_diagnostics.py::test_masked_plan_diagnostics_vs_fp64_oracle."""
    from svdq_amd.mask_loader import MaskSet
    key = (n, fp16, inverted, center, max_rank)
    if key not in _MASKED:
        dev = _dev()
        ft, base, delta = _checkpoints(MSIZES, n, torch.float32, 500)
        gen = torch.Generator().manual_seed(100 + n)
        masks = [(torch.rand(D, generator=gen) < q) for D, q in zip(MSIZES, MDENS)]
        sel = [(~m if inverted else m) for m in masks]
        ms = MaskSet(MSIZES, dev)
        ct, cf = ms.count_scan([m.to(dev) for m in masks])
        comb = ms._s["mb"]
        rows_dev = cf if inverted else ct
        plan = _plan(sq, MSIZES, n, fp16, center, max_rank=max_rank)
        mtab = _table(comb)
        us = ms.unit_starts(plan, rows_dev, entry_map=[(q, inverted) for q in range(len(MSIZES))])
        comp = [[torch.cat([v[s.to(dev)], torch.zeros(D - int(s.sum()), device=dev)]) for v in vs]
                for vs, s, D in zip(delta, sel, MSIZES)]
        plan.run(plan.pointer_table(comp), rows_dev)
        sm = plan.fetch_small()
        assert [int(x) for x in sm.rows] == [int(s.sum()) for s in sel]
        ftab, btab = _table([f for fs in ft for f in fs]), _table(base)
        got = plan.diagnostics_masked_from_base(ftab, btab, mtab, us, rows_dev).cpu().numpy()
        want = plan.diagnostics_masked(_table([d for ds in delta for d in ds]), mtab, us, rows_dev).cpu().numpy()
        _MASKED[key] = (plan, sm, delta, sel, got, want, (ms, comb, ft, base, mtab, us, rows_dev, ftab, btab))
    return _MASKED[key]


@pytest.mark.parametrize("n_tasks", [4, 8, 16, 20, 32])
@pytest.mark.parametrize("inverted", [False, True])
def test_masked_from_base_is_bit_for_bit_the_materialised_deltas(sq, n_tasks, inverted):
    plan, sm, delta, sel, got, want, _ = _masked(sq, n_tasks, n_tasks % 8 != 0, inverted)
    assert got.shape == (len(MSIZES), n_tasks, 6)
    assert _same(got, want)
    assert np.isfinite(want).any()


# ------------------------------------------------------------------------------------------ 4. truth
def _host_artifacts(orc, plan, sm, p, t):
    """The device's own artifacts of (parameter p, task t) on the host, dequantized by the oracle."""
    k, r, rows = int(sm.k[p]), int(sm.r[p]), int(sm.rows[p])
    Uh, Ul, mean = plan.basis_tensors(p, k, r, rows)
    ch = torch.from_numpy(sm.c_high[p, t, :k].astype(np.float32))
    nl = r - k
    if nl > 0:
        cl = torch.from_numpy(orc.rtvq_dequantize({"codes": sm.codes[p, t, :, :nl], "scale": sm.scale[p, t],
                                                   "zero_point": sm.zero_point[p, t]}).reshape(-1).copy())
    else:
        cl = torch.zeros(0)
    return Uh.cpu(), Ul.cpu(), ch, cl, (mean.cpu() if mean is not None else None)


# (center, max_rank) per task count.  The spikes carry most of the energy, so at the 0.9 threshold of the other tests a
# small plan keeps k = r - 1 columns and its quantizer input is the degenerate one.  With these settings the
# oracle alone (compress_parameter on the CPU, these seeds) leaves finite: N = 4 32/32 plain and 24/24 masked, N = 8
# 59/64 and 48/48, N = 20 160/160 and 120/120 -- with (False, None) at N = 4 and 8 it is 20/32, 16/24, 40/64, 29/48.
TRUTH_SETTINGS = {4: (False, 1), 8: (True, None), 20: (False, None)}


@pytest.mark.parametrize("n_tasks", [4, 8, 20])
@pytest.mark.parametrize("masked", [False, True])
def test_from_base_numbers_vs_fp64_formula(sq, n_tasks, masked):
    """Every finite tuple against the fp64 evaluation of diagnostics.py:72-117, 186-215 on x = ft.float() - base.float()
    (or x[sel]); a tuple is excused only where the quantizer's input is degenerate (r - k <= 2 or D < N), and
    at least three quarters of the (parameter, task) pairs are checked."""
    from oracle import svd_hybrid_oracle as orc
    center, max_rank = TRUTH_SETTINGS[n_tasks]
    if masked:
        plan, sm, delta, sel, got, want, _ = _masked(sq, n_tasks, n_tasks % 8 != 0, False, center, max_rank)
        sizes = MSIZES
    else:
        plan, ft, base, delta, ftab, btab, got, want = _plain(sq, n_tasks, True, center, max_rank)
        sm, sel, sizes = plan.fetch_small(), None, SIZES
    assert _same(got, want)
    finite = 0
    for p, D in enumerate(sizes):
        for t in range(n_tasks):
            Uh, Ul, ch, cl, _ = _host_artifacts(orc, plan, sm, p, t)
            if not (torch.isfinite(cl).all() and np.isfinite(got[p, t]).all()):
                assert int(sm.r[p]) - int(sm.k[p]) <= 2 or D < n_tasks
                continue
            x = delta[p][t].cpu()
            if sel is not None:
                x = x[sel[p]]
            diag_check(dict(zip(orc.DIAG_KEYS, got[p, t])), x, Uh, Ul, ch, cl, what=("from_base", masked, p, t))
            finite += 1
    assert finite >= 0.75 * len(sizes) * n_tasks, (finite, len(sizes) * n_tasks)


# ------------------------------------------------------------------------------------------ 5. a base that matters
def test_a_permuted_base_table_changes_the_result(sq):
    sizes = [4096 + 37, 300, 4096 + 37]
    ft, base, delta = _checkpoints(sizes, 8, torch.float32, 900)
    plan = _plan(sq, sizes, 8, True, False)
    ftab, btab = plan.pointer_table(ft), _table(base)
    plan.run_from_base(ftab, btab)
    right = plan.diagnostics_from_base(ftab, btab).cpu().numpy()
    assert _same(right, plan.diagnostics(_table([d for ds in delta for d in ds])).cpu().numpy())
    swapped = plan.diagnostics_from_base(ftab, _table([base[2], base[1], base[0]])).cpu().numpy()
    assert _same(swapped[1], right[1])
    for p in (0, 2):
        assert not np.array_equal(swapped[p, :, 4], right[p, :, 4])      # original_norm: ||ft - the other base||
        want = [float((f.double() - base[2 - p].double()).norm()) for f in ft[p]]
        assert np.allclose(swapped[p, :, 4], want, rtol=1e-5)
    plan.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_output_untouched(sq):
    nat = sq._native
    lib = nat.lib()
    plan, ft, base, delta, ftab, btab, _, _ = _plain(sq, 8, True, True)
    out = torch.full((plan.P, plan.N, 6), -7.0, dtype=torch.float64, device=_dev())
    work = torch.empty(int(lib.svdq_diagnostics_work_bytes(plan._h)), dtype=torch.uint8, device=_dev())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.svdq_diagnostics_from_base(plan._h, p(ftab), None, None, p(plan.small), p(plan.basis), p(plan.mean), 0, p(out),
                                        p(work), st)
    assert rc == nat.SVDQ_EINVAL and "base_ptrs" in nat.last_error()
    rc = lib.svdq_diagnostics_masked_from_base(plan._h, p(ftab), None, p(ftab), p(ftab), p(ftab), p(plan.small),
                                               p(plan.basis), p(plan.mean), 0, p(out), p(work), st)
    assert rc == nat.SVDQ_EINVAL and "base_ptrs" in nat.last_error()
    rc = lib.svdq_diagnostics_masked_from_base(plan._h, p(ftab), p(btab), None, None, None, p(plan.small), p(plan.basis),
                                               p(plan.mean), 0, p(out), p(work), st)
    assert rc == nat.SVDQ_EINVAL and "mask_ptrs" in nat.last_error()
    with pytest.raises(ValueError, match="base_ptrs"):
        plan.diagnostics_from_base(ftab, None)
    # the masked form on a half plan: the error svdq_diagnostics_masked gives
    half = _plan(sq, [64], 8, True, True, torch.bfloat16)
    hp = ctypes.c_void_p(half._h.value)
    rc_m = lib.svdq_diagnostics_masked(hp, p(ftab), p(ftab), p(ftab), p(ftab), p(plan.small), p(plan.basis), p(plan.mean), 0,
                                       p(out), p(work), st)
    msg_m = nat.last_error()
    rc_b = lib.svdq_diagnostics_masked_from_base(hp, p(ftab), p(btab), p(ftab), p(ftab), p(ftab), p(plan.small),
                                                 p(plan.basis), p(plan.mean), 0, p(out), p(work), st)
    msg_b = nat.last_error()
    assert rc_m == rc_b == nat.SVDQ_EUNSUPPORTED
    assert msg_b == msg_m.replace("svdq_diagnostics_masked", "svdq_diagnostics_masked_from_base")
    half.close()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------ 7. / 8. dictionary API
def _model(sq, tmp_path=None):
    """3 parameters x 4 tasks, one of them masked; checkpoints on the device in fp32."""
    from oracle import svd_hybrid_oracle as orc
    dev = _dev()
    tasks = ["t3", "t1", "t2", "t0"]
    shapes = {"a.weight": (96, 64), "b.bias": (257,), "c.weight": (128, 70)}
    g = torch.Generator().manual_seed(77)
    base = {n: torch.randn(s, generator=g).to(dev) for n, s in shapes.items()}
    ft = {t: {} for t in tasks}
    for i, (n, s) in enumerate(shapes.items()):
        for t, d in zip(tasks, orc.synthetic_deltas(int(np.prod(s)), len(tasks), 40 + i, rank=3)):
            ft[t][n] = base[n] + d.view(s).to(dev)
    masks = {"c.weight": (torch.rand(shapes["c.weight"], generator=g) < 0.7).to(dev)}
    deltas = {t: {n: ft[t][n] - base[n] for n in shapes} for t in tasks}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2)
    return tasks, shapes, base, ft, masks, deltas, cfg


def _assert_same_dict(a, b, path=""):
    assert type(a) is type(b) or (isinstance(a, (int, float, np.integer, np.floating)) and
                                  isinstance(b, (int, float, np.integer, np.floating))), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), (path, list(a.keys()), list(b.keys()))
        for k in a:
            _assert_same_dict(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same_dict(x, y, f"{path}[{i}]")
    elif isinstance(a, float) and a != a:
        assert b != b, path
    else:
        assert a == b, (path, a, b)


def test_adopted_artifacts_give_the_original_runs_diagnostics(sq, tmp_path):
    tasks, shapes, base, ft, masks, deltas, cfg = _model(sq)
    bases, comp = sq.run_basis_and_compress(deltas, masks, cfg, "cuda")
    from svdq_amd import diagnostics as dg
    assert sorted(dg._batched_errors(deltas, comp, bases, masks)) == sorted(shapes)      # the same kernels on both sides
    want = sq.compute_all_diagnostics(deltas, comp, bases, masks, cfg, device="cuda")
    d = str(tmp_path / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()}}, cfg, d)
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda", masks=masks)
    assert sorted(dg._checkpoint_errors(base, ft, ac, ab, masks)) == sorted(shapes)      # all three at plan level
    got = sq.compute_all_diagnostics_from_checkpoints(base, ft, ac, ab, masks, cfg, device="cuda")
    _assert_same_dict(got, want)


def test_dictionary_api_on_a_from_base_run_with_a_forced_fallback(sq):
    tasks, shapes, base, ft, masks, deltas, cfg = _model(sq)
    bases, comp = sq.run_basis_and_compress_from_checkpoints(base, ft, cfg, "cuda", combined_masks=masks)
    from svdq_amd import diagnostics as dg
    assert sorted(dg._checkpoint_errors(base, ft, comp, bases, masks)) == sorted(shapes)
    whole = sq.compute_all_diagnostics_from_checkpoints(base, ft, comp, bases, masks, cfg, device="cuda")
    ref_b, ref_c = sq.run_basis_and_compress(deltas, masks, cfg, "cuda")
    _assert_same_dict(whole, sq.compute_all_diagnostics(deltas, ref_c, ref_b, masks, cfg, device="cuda"))
    # a mask that is not the tensor the run compressed with: that one parameter goes per parameter
    foreign = {"c.weight": masks["c.weight"].clone()}
    assert sorted(dg._checkpoint_errors(base, ft, comp, bases, foreign)) == ["a.weight", "b.bias"]
    got = sq.compute_all_diagnostics_from_checkpoints(base, ft, comp, bases, foreign, cfg, device="cuda")
    assert list(got["per_parameter"]) == sorted(shapes) and got["summary"]["num_parameters"] == len(shapes)
    for n in ("a.weight", "b.bias"):
        _assert_same_dict(got["per_parameter"][n], whole["per_parameter"][n])
    quant = sq.RTVQQuantizer(num_bits=cfg.svd_low_bits, num_stages=cfg.svd_rtvq_stages)
    one = {t: {"c.weight": ft[t]["c.weight"].float() - base["c.weight"].float()} for t in tasks}
    want = sq.compute_parameter_diagnostics("c.weight", one, comp["c.weight"], bases["c.weight"], foreign["c.weight"],
                                            quant, "cuda")
    _assert_same_dict(got["per_parameter"]["c.weight"], want)
    assert list(want["reconstruction_errors"]) == tasks


# ------------------------------------------------------------------------------------------ 9. operator
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_operator_equals_the_ctypes_call(sq, dtype):
    n = 8
    ft, base, delta = _checkpoints(SIZES, n, dtype, 620)
    plan = _plan(sq, SIZES, n, True, True, dtype)
    ftab, btab = plan.pointer_table(ft), _table(base)
    plan.run_from_base(ftab, btab)
    want = plan.diagnostics_from_base(ftab, btab)
    flat = [f for fs in ft for f in fs]
    small, basis, mean = torch.ops.svdq.compress_from_base(flat, base, n, 0.9, 0, True, True, 4, 2)
    got = torch.ops.svdq.diagnostics_from_base(flat, base, small, basis, mean, n, 0.9, 0, True, True, 4, 2, False)
    assert got.dtype == torch.float64 and _same(got.cpu().numpy(), want.cpu().numpy())
    with pytest.raises(ValueError, match="one base tensor per parameter"):
        torch.ops.svdq.diagnostics_from_base(flat, base[:-1], small, basis, mean, n, 0.9, 0, True, True, 4, 2, False)
    plan.close()


# ------------------------------------------------------------------------------------------ 10. graph capture
@pytest.mark.parametrize("n_tasks", [8, 20])
def test_capture_and_replay_give_the_eager_bits(sq, n_tasks):
    plan, ft, base, delta, ftab, btab, eager, _ = _plain(sq, n_tasks, True, True)
    lib = sq._native.lib()
    dev = _dev()
    out = torch.full((plan.P, plan.N, 6), -7.0, dtype=torch.float64, device=dev)
    work = torch.empty(int(lib.svdq_diagnostics_work_bytes(plan._h)), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        sq._native.check(lib.svdq_diagnostics_from_base(plan._h, p(ftab), p(btab), None, p(plan.small), p(plan.basis),
                                                        p(plan.mean), 0, p(out), p(work), st), "svdq_diagnostics_from_base")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), eager)
    out.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())      # capture does not execute
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), eager)
