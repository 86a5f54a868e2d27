"""
CPU checks of tests/basis_ops_model.py: the derived bounds of ``svdq_project``, ``svdq_reconstruct`` and the six numbers
of ``svdq_recon_error`` hold for three legitimate fp32 evaluations at every case the GPU tests run (the launch geometry
included), and they are sharp enough to matter -- each mistake a kernel of this shape could plausibly make exceeds them
on a spiked row.  No GPU, no library call.
"""
import pytest
import torch

import basis_ops_model as bm
from helpers import diag_check, diag_check_given

SCALE = 0.5
# every case the GPU tests run: every row count with every pair, and the two long row counts (8 and 9 rows per thread)
# at k + nl <= 2
CASES = [(rows, k, nl) for rows in bm.ROWS for k, nl in bm.PAIRS] + \
        [(rows, k, nl) for rows in bm.ROWS_HUGE for k, nl in bm.PAIRS_SMALL if k + nl <= 2]
MUTATION_PAIRS = [(1, 1), (2, 2), (7, 9)]      # k >= 1 and nl >= 1: every mutation applies


def _id(c):
    return "rows%d-k%d-nl%d" % c


_CASES = {}


def _case(rows, k, nl, fp16):
    key = (rows, k, nl, fp16)
    if key not in _CASES:
        _CASES[key] = bm.Case(rows, k, nl, fp16)
    return _CASES[key]


def test_the_geometry_is_the_kernels():
    """grid and rows per thread at the edges the issue names: a second row above 256 rows, a second block above 2048, a
    ninth row above 1024 * 2048."""
    assert [bm.grid(r) for r in (1, 256, 2048, 2049, 4096, 4097)] == [1, 1, 1, 2, 2, 3]
    assert [bm.rows_per_thread(r) for r in (1, 256, 257, 2048, 2049, 4097)] == [1, 1, 2, 8, 5, 6]
    assert bm.grid(bm.ROWS_HUGE[0]) == bm.grid(bm.ROWS_HUGE[1]) == 1024
    assert [bm.rows_per_thread(r) for r in bm.ROWS_HUGE] == [8, 9]
    assert bm.spike_rows(4097) == [0, 255, 256, 2047, 2048, 4096] and bm.spike_rows(2) == [0, 1]
    assert len(bm.PAIRS_SMALL) == 14 and all(1 <= k + nl <= 4 for k, nl in bm.PAIRS_SMALL)
    c = _case(4097, 2, 2, True)
    typ = float(c.U64().abs().median())
    for s in bm.spike_rows(4097):      # 1e3 x the typical magnitude, in U, the mean and orig
        assert float(c.U64()[s].abs().min()) > 500 * typ
        assert abs(float(c.mean[s])) > 500 * float(c.mean.abs().median())
        assert abs(float(c.orig[s])) > 500 * float(c.orig.abs().median())


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_legitimate_fp32_evaluations_stay_inside_the_bounds(case, fp16):
    c = _case(*case, fp16)
    for use_mean in (False, True):
        mean = c.mean if use_mean else None
        want, bound = bm.project_exact(c.U_high, c.U_low, c.delta, mean)
        out, obound = bm.reconstruct_exact(c.U_high, c.U_low, c.coef, mean, SCALE)
        for order in bm.ORDERS:
            got = torch.from_numpy(bm.project_fp32(c, use_mean, order)).double()
            assert bool(((got - want).abs() <= bound).all()), ("project", order, use_mean, (got - want).abs() / bound)
            got = torch.from_numpy(bm.reconstruct_fp32(c, use_mean, SCALE, order)).double()
            assert bool(((got - out).abs() <= obound).all()), ("reconstruct", order, use_mean)
            diag_check(bm.six_fp32(c, use_mean, order), c.orig, c.U_high, c.U_low, c.c_high(), c.c_low(),
                       what=("recon_error", order, use_mean), mean=mean)
    rec = torch.from_numpy(bm._rec_fp32(c, True, "kernel"))
    diag_check_given(bm.six_from(rec.numpy(), c.orig.numpy()), c.orig, rec, what="given reconstruction")


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("pair", MUTATION_PAIRS, ids=lambda p: "k%d-nl%d" % p)
def test_every_mutation_exceeds_the_bounds_on_a_spiked_row(pair, fp16):
    """A dropped row, a doubled row, the k / nl split off by one, the mean omitted, the mean added after ``* scale`` and
    row d read with stride k + 1, each evaluated EXACTLY: it is the mistake, not rounding, that has to exceed the
    bound.  Dropped and doubled rows are tried at every spiked row (0, 255, 256, 2047, 2048 and the last)."""
    c = _case(4097, *pair, fp16)
    want, bound = bm.project_exact(c.U_high, c.U_low, c.delta, c.mean)
    out, obound = bm.reconstruct_exact(c.U_high, c.U_low, c.coef, c.mean, SCALE)
    spikes = bm.spike_rows(c.rows)
    assert spikes == [0, 255, 256, 2047, 2048, 4096]

    def six_exceeds(got):
        return max(bm.six_ratio(got, c.orig, c.U_high, c.U_low, c.c_high(), c.c_low(), mean=c.mean).values()) > 1.0

    # the unmutated exact values pass, so what follows is the mutation's doing
    assert not six_exceeds(bm.six_mutated(c, None))
    assert bool(((bm.rec_mutated(c, None, scale=SCALE) - out).abs() <= obound).all())
    for mutation in bm.MUTATIONS:
        for row in (spikes if mutation in ("drop_row", "double_row") else [None]):
            if mutation != "mean_after_scale":      # the projection has no scale
                got = bm.project_mutated(c, mutation, row)
                assert bool(((got - want).abs() > bound).any()), ("project", mutation, row)
            got = bm.rec_mutated(c, mutation, row, scale=SCALE)
            bad = (got - out).abs() > obound
            if mutation == "drop_row":
                assert bool(bad[row]), ("reconstruct", mutation, row)
            elif mutation == "double_row":
                assert bool(bad[row + 1 if row + 1 < c.rows else row - 1]), ("reconstruct", mutation, row)
            else:
                assert any(bool(bad[s]) for s in spikes), ("reconstruct", mutation)
            if mutation != "mean_after_scale":      # the error has no scale
                assert six_exceeds(bm.six_mutated(c, mutation, row)), ("recon_error", mutation, row)


def test_the_nonfinite_pattern_is_torchs():
    """What the GPU tests expect for a NaN or an Inf among the operands, on the model's own fp32 evaluation: every
    number's class is the one torch gives on the CPU; a NaN in orig leaves ``relative_error`` 0 (``nan > 1e-10`` is
    False at diagnostics.py:96) beside a NaN ``absolute_error`` and a NaN maximum, wherever the NaN sits."""
    c = _case(2048, 2, 2, True)
    for row in (0, 256, 1000, 2047):
        x = c.orig.clone()
        x[row] = float("nan")
        got = bm.six_from(bm._rec_fp32(c, False, "kernel"), x.numpy())
        pattern = bm.check_six_nonfinite(got, x, c.U_high, c.U_low, c.c_high(), c.c_low())
        assert pattern == {"absolute_error": "nan", "relative_error": "finite", "max_absolute_error": "nan",
                           "mean_absolute_error": "nan", "original_norm": "nan", "reconstructed_norm": "finite"}
        lost = dict(got, max_absolute_error=1.0)      # a maximum that lost the NaN is caught
        with pytest.raises(AssertionError):
            bm.check_six_nonfinite(lost, x, c.U_high, c.U_low, c.c_high(), c.c_low())
    x = c.orig.clone()
    x[5] = float("inf")
    got = bm.six_from(bm._rec_fp32(c, False, "kernel"), x.numpy())
    pattern = bm.check_six_nonfinite(got, x, c.U_high, c.U_low, c.c_high(), c.c_low())
    assert pattern == {"absolute_error": "+inf", "relative_error": "nan", "max_absolute_error": "+inf",
                       "mean_absolute_error": "+inf", "original_norm": "+inf", "reconstructed_norm": "finite"}
