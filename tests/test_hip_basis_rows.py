"""
Row-exact tests of what pass 2 of the compressor writes -- the basis ``U = [U_high | U_low]`` and the row mean -- for
every kernel variant the launchers can select (run with ``-m gpu`` on an MI355X).

Every consumer test in this suite (merge, diagnostics, artifacts, reload) evaluates its formula on the artifacts the
kernel read, and every alternative input route is tested as bit-identical to the plain fp32 run; the plain run itself
was seen row by row only on the golden chains (D <= 65 536) and through aggregates (MSE, spans, norms) everywhere else.
A block written to the wrong rows, an unwritten tail or two swapped rows changes those aggregates by ~1/D.  Here the
truth is the input itself: ``helpers.basis_rows_check`` evaluates, in fp64 on the host,

  (a) T[i, t] = mean[i] + sum_j U[i, j] coef[t, j]      element by element, against a forward-error bound,
  (b) mean[i] against the fp64 row mean,                 every row,
  (c) U^T U = I over all rows                            (zero columns exactly zero),

with ``coef`` the device's own fp32 coefficients before rounding -- no sign, rotation or quantizer freedom.  The bounds
are derived (helpers.basis_rows_ratios states them) except g and c, fitted on the REFERENCE chain on the CPU (LAPACK
fp32 SVD, ``.half()``, fp32 GEMVs) over the shapes of this module as twice what the reference needs
(helpers.BASIS_ROWS_G0, BASIS_ROWS_G, BASIS_ROWS_C; tools/fit_basis_rows.py regenerates the figures, DESIGN.md section 2
discusses them):

  largest figure over every (parameter, variant)                   fp16 basis      fp32 basis
  reference chain (CPU, 4 threads), 3 192 chains up to D = 70 001 + the four of D = 4 194 307 (in brackets)
  (a) error / bound without the g term                             0.93 (1.72)     38.7 (506)
      g needed below 64 rows -> committed (flat)                   0 -> 0          24.32 -> 48.64
      g needed from 64 rows on, in sqrt(D) -> committed            0 (3.26) -> 6.52    5.51 (3.65) -> 11.02
  (b) error / bound                                                0.58            0.58
  (c) |U^T U - I|                                                  6.3e-4 (3.3e-4) 1.8e-6 (1.0e-5)
      c needed -> committed                                        0 -> 281        17.0 (140.5) -> 281
  device (MI355X), 3 901 checked parameters, measured after the constants were fixed
  (a) error / bound (without the g term: g needed = 0)             0.93 (0.93)     0.08 (0.38)
  (b) error / bound                                                0.585           0.585
  (c) error / bound (c needed)                                     0.63 (0.4)      0.12 (33.5: N = 17, D = 255, centred --
      above the reference's 17.0 at D <= 70 001: the eps32 sigma_0 / sigma_i of a column formed as Tc w_i / sigma_i)
  The module runs in about 40 s (198 tests).

tests/test_basis_rows_cpu.py repeats that measurement on a reduced list without a GPU and shows that a dropped row, two
swapped rows, a block shifted by one row and an unwritten mean tail each exceed the bounds at least twentyfold.
Inputs: ``synthetic_deltas`` plus task-dependent spikes at tile, block, unit and tensor boundaries.
"""
import numpy as np
import pytest
import torch

from helpers import (BASIS_ROWS_N, BASIS_ROWS_LARGE, basis_rows_sizes, basis_rows_inputs, basis_rows_ratios,
                     basis_rows_assert)

pytestmark = pytest.mark.gpu
SETTINGS = dict(energy_threshold=0.9, max_rank=None, low_bits=4, rtvq_stages=2)


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle
    return svd_hybrid_oracle


def _dev():
    return torch.device("cuda", 0)


def check_parameter(plan, sm, p, deltas, D, what, chunk=1 << 18):
    """The three identities on parameter ``p`` of a finished plan against the host fp32 inputs ``deltas`` (N CPU
    tensors of D rows), then what is cheap: ranks, row count, shapes / dtypes / contiguity, sigma order, fp16 c_high."""
    N, fp16, center = plan.N, plan.fp16, plan.center
    k, r, rows = int(sm.k[p]), int(sm.r[p]), int(sm.rows[p])
    assert rows == D and r == min(D, N) and 1 <= k <= r, (what, rows, r, k)
    U_high, U_low, mean = plan.basis_tensors(p, k, r, rows)
    dt = torch.float16 if fp16 else torch.float32
    assert U_high.shape == (D, k) and U_low.shape == (D, r - k), what
    assert U_high.dtype == dt and U_low.dtype == dt and U_high.is_contiguous() and U_low.is_contiguous(), what
    if center:
        assert mean.shape == (D, 1) and mean.dtype == torch.float32 and mean.is_contiguous(), what
    else:
        assert mean is None, what
    sigma = sm.sigma[p, :r]
    assert np.all(np.isfinite(sigma)) and np.all(sigma[:-1] >= sigma[1:]) and sigma[-1] >= 0.0, (what, sigma)
    coef = sm.coef[p, :N, :r]
    c16 = torch.from_numpy(coef[:, :k].copy()).half().numpy()
    assert np.array_equal(sm.c_high[p, :N, :k].view(np.uint16), c16.view(np.uint16)), what
    s = basis_rows_ratios(deltas, U_high.cpu(), U_low.cpu(), mean.cpu() if center else None, coef, sigma, fp16, center,
                          chunk=chunk)
    print(f"basis_rows {what} a={s['a']:.3f} a0={s['a0']:.3f} g_need={s['a_need']:.3f} b={s['b']:.3f} c={s['c']:.3f} "
          f"c_need={s['c_need']:.2f} c_err={s['c_err']:.2e}")      # every figure, before anything asserts on it
    basis_rows_assert(s, what)
    return s


# ------------------------------------------------------------------------------------------------ the anchor
VARIANTS = [(N, fp16, center, unit_rows, 0) for N in BASIS_ROWS_N for fp16 in (True, False) for center in (True, False)
            for unit_rows in (0, 1024)]
# N = 17..20: the default pass 2 is k_basis_project_q (columns 16..19 through 4x4-block MFMAs); plan flag 8 selects the
# two-wave kernel every other N > 16 runs
VARIANTS += [(N, fp16, center, unit_rows, 8) for N in BASIS_ROWS_N if 16 < N <= 20 for fp16 in (True, False)
             for center in (True, False) for unit_rows in (0, 1024)]


@pytest.mark.parametrize("N,fp16,center,unit_rows,flags", VARIANTS)
def test_rows_every_pass2_variant(sq, orc, N, fp16, center, unit_rows, flags):
    """One ragged plan per variant: every NTP in {4, ..., 32} with N == NTP (the FULL kernels) and N < NTP, both
    storage types, centred or not, auto and 1024-row units; later parameters exercise slab and mean offsets."""
    from svdq_amd.pipeline import CompressPlan
    dev = _dev()
    sizes = basis_rows_sizes(N)
    host = [basis_rows_inputs(orc, D, N, unit_rows) for D in sizes]
    vecs = [[d.to(dev) for d in ds] for ds in host]
    plan = CompressPlan(sizes, N, center=center, fp16=fp16, device=dev, unit_rows=unit_rows, flags=flags, **SETTINGS)
    plan.run(plan.pointer_table(vecs))
    torch.cuda.synchronize()
    sm = plan.fetch_small()
    for p, D in enumerate(sizes):
        check_parameter(plan, sm, p, host[p], D, f"N={N} fp16={fp16} center={center} unit_rows={unit_rows} "
                                                  f"flags={flags} p={p} D={D}")
    plan.close()


@pytest.mark.parametrize("D,N,fp16,center", BASIS_ROWS_LARGE)
def test_rows_large_single_parameter(sq, orc, D, N, fp16, center):
    """Many units and an unaligned tail; the checker runs in row chunks, so host memory stays flat."""
    from svdq_amd.pipeline import CompressPlan
    dev = _dev()
    host = basis_rows_inputs(orc, D, N, 0)
    vecs = [[d.to(dev) for d in host]]
    plan = CompressPlan([D], N, center=center, fp16=fp16, device=dev, **SETTINGS)
    plan.run(plan.pointer_table(vecs))
    torch.cuda.synchronize()
    sm = plan.fetch_small()
    check_parameter(plan, sm, 0, host, D, f"large N={N} fp16={fp16} center={center} D={D}")
    plan.close()


# ------------------------------------------------------------------------------------------------ the other routes
ROUTE_SIZES = [257, 4101, 70001]
ROUTE_CASES = [(5, True, True), (8, False, True), (16, True, False), (20, True, True), (32, False, False)]


def _table(tensors, dev):
    return torch.tensor([x.data_ptr() for x in tensors], dtype=torch.int64).to(dev)


def _adopt(sq, rows, N, fp16, center, small, basis, mean):
    """A plan object over the packed buffers a torch op returned, for fetch_small / basis_tensors."""
    plan = sq.pipeline.CompressPlan(rows, N, center=center, fp16=fp16, device=_dev(), gram_only=True, **SETTINGS)
    plan.small, plan.basis, plan.mean = small, basis, (mean if center else None)
    return plan


@pytest.mark.parametrize("N,fp16,center", ROUTE_CASES)
@pytest.mark.parametrize("density", [0.2, 0.94])
def test_rows_other_routes(sq, orc, N, fp16, center, density):
    """Gather, mask walk (both polarities), minus-base, gather-from-base and fp16 / bf16 inputs, each checked against
    the host-compacted / host-differenced fp32 input -- directly, not through their bit-identity with the plain run."""
    from svdq_amd.pipeline import CompressPlan
    from svdq_amd.mask_loader import MaskSet
    dev = _dev()
    sizes = ROUTE_SIZES
    g = torch.Generator().manual_seed(1000 * N + int(100 * density))
    host = [basis_rows_inputs(orc, D, N, 0) for D in sizes]
    vecs = [[d.to(dev) for d in ds] for ds in host]
    masks_h = [torch.rand(D, generator=g) < density for D in sizes]
    masks = [m.to(dev) for m in masks_h]
    kw = dict(center=center, fp16=fp16, device=dev, **SETTINGS)
    tag = f"N={N} fp16={fp16} center={center} density={density}"

    def check_all(plan, inputs, counts, route):
        torch.cuda.synchronize()
        sm = plan.fetch_small()
        for p in range(len(sizes)):
            check_parameter(plan, sm, p, inputs[p], counts[p], f"{route} {tag} p={p} rows={counts[p]}")
        plan.close()

    ms, mw = MaskSet(sizes, dev), MaskSet(sizes, dev)
    it, if_, ct, cf = ms.indices(masks, want_false=True)
    ct2, cf2 = mw.count_scan(masks)
    assert torch.equal(ct, ct2) and torch.equal(cf, cf2)
    mtab = _table(mw._s["mb"], dev)
    for inv, idx, cnt in ((False, it, ct), (True, if_, cf)):
        sel = [(~m if inv else m) for m in masks_h]
        compact = [[d[s] for d in ds] for ds, s in zip(host, sel)]
        counts = [int(s.sum()) for s in sel]
        assert counts == cnt.cpu().tolist()
        # index lists
        ga = CompressPlan(sizes, N, **kw)
        ga.run_gather(ga.pointer_table(vecs), _table(idx, dev), cnt)
        check_all(ga, compact, counts, f"gather inv={inv}")
        # mask walk: N <= 16 on the walk forms of the two passes, above on the one-wave kernels
        wk = CompressPlan(sizes, N, **kw)
        us = mw.unit_starts(wk, cnt, entry_map=[(q, inv) for q in range(len(sizes))] if inv else None)
        wk.run_masked(wk.pointer_table(vecs), mtab, us, cnt)
        check_all(wk, compact, counts, f"walk inv={inv}")
    mw.close()
    # minus-base: the input of the identity is fl32(finetuned - base), formed on the host in fp32
    base_h = [torch.randn(D, generator=g) for D in sizes]
    ft_h = [[b + d for d in ds] for b, ds in zip(base_h, host)]
    diff = [[f - b for f in fs] for b, fs in zip(base_h, ft_h)]
    base = [b.to(dev) for b in base_h]
    ft = [[f.to(dev) for f in fs] for fs in ft_h]
    for inv, idx, cnt in ((False, it, ct), (True, if_, cf)):
        sel = [(~m if inv else m) for m in masks_h]
        gb = CompressPlan(sizes, N, **kw)
        gb.run_gather_from_base(gb.pointer_table(ft), _table(base, dev), _table(idx, dev), cnt)
        check_all(gb, [[d[s] for d in ds] for ds, s in zip(diff, sel)], [int(s.sum()) for s in sel],
                  f"gather_from_base inv={inv}")
    ms.close()
    if density != 0.2:      # what follows has no mask: once per (N, fp16, center)
        return
    fb = CompressPlan(sizes, N, **kw)
    fb.run_from_base(fb.pointer_table(ft), _table(base, dev))
    check_all(fb, diff, sizes, "from_base")
    # fp16 / bf16 task tensors read as they are: the identity's input is their exact fp32 value
    for dtype in (torch.float16, torch.bfloat16):
        half_h = [[d.to(dtype) for d in ds] for ds in host]
        half = [v.to(dev) for vs in half_h for v in vs]
        out = torch.ops.svdq.compress(half, N, SETTINGS["energy_threshold"], 0, center, fp16, SETTINGS["low_bits"],
                                      SETTINGS["rtvq_stages"])
        check_all(_adopt(sq, sizes, N, fp16, center, *out), [[v.float() for v in vs] for vs in half_h], sizes,
                  f"op {str(dtype).replace('torch.', '')}")
