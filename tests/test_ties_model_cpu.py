"""
The numpy model of the TIES merge (tests/ties_model.py) against an independent torch restatement of the published steps
(Yadav et al. 2023: topk_values_mask with kthvalue, resolve_sign with sign(sum), disjoint_merge with where), plus hand
cases for the places the definition is sharp: a magnitude tie at the threshold, exact cancellation, density 1.

Thresholds and kept counts must be equal exactly.  Merged values may differ in the last bits: torch's reductions add in
another order than the model's task-by-task loop.  Each of the two sums of T terms is within (T - 1) 2^-24 sum|v| of the
exact one, so the sums differ by less than T 2^-23 sum|v|; the division by a count >= 1 only shrinks that.
"""
import numpy as np
import pytest
import torch

import ties_model as tm

D = 20011


def _published(v: torch.Tensor, density: float, merge_func: str):
    """The published steps on a [T, D] tensor; s == 0 elects positive (the one deliberate difference)."""
    T, d = v.shape
    k = max(d - int(d * density), 1)
    kth = v.abs().kthvalue(k, dim=1, keepdim=True).values
    mask = v.abs() >= kth
    trimmed = v * mask
    sign = torch.sign(trimmed.sum(dim=0))
    sign[sign == 0] = 1
    rows = torch.where(sign.unsqueeze(0) > 0, trimmed > 0, trimmed < 0)
    sel = trimmed * rows
    if merge_func == "mean":
        merged = sel.sum(dim=0) / torch.clamp((sel != 0).sum(dim=0).float(), min=1)
    else:
        merged = sel.sum(dim=0)
    return merged, kth.view(-1), mask.sum(dim=1)


@pytest.mark.parametrize("merge_func", ["mean", "sum"])
@pytest.mark.parametrize("density", [0.001, 0.2, 0.5, 1.0])
@pytest.mark.parametrize("T", [1, 3, 8, 20])
def test_model_matches_the_published_steps(T, density, merge_func):
    g = torch.Generator().manual_seed(1000 * T + int(1000 * density))
    v = torch.randn(T, D, generator=g)
    want, kth, kept = _published(v, density, merge_func)
    got, stats = tm.ties_merge(v.numpy(), density, merge_func)
    assert np.array_equal(stats["thresholds"].view(np.uint32), kth.numpy().view(np.uint32))
    assert np.array_equal(stats["kept"], kept.numpy())
    assert stats["rows"] == D and int(kept.sum()) >= T * int(D * density)
    bound = T * 2.0 ** -23 * v.abs().sum(dim=0).double().numpy()
    err = np.abs(got.astype(np.float64) - want.double().numpy())
    assert (err <= bound).all(), float((err - bound).max())
    # the counters restated: a row is empty when the trim keeps nothing of it
    assert stats["empty_rows"] == int((~(v.abs() >= kth.view(-1, 1)).any(dim=0)).sum())


def test_a_magnitude_tie_at_the_threshold_keeps_every_equal_value():
    v = np.array([[1, -2, 2, 3, -2, 0.5, 2, -4]], dtype=np.float32)
    # density 0.25: keep_n = 2, j = 6 -> tau = the 6th smallest of {0.5, 1, 2, 2, 2, 2, 3, 4} = 2: six values are kept
    out, st = tm.ties_merge(v, 0.25)
    assert st["thresholds"][0] == 2 and st["kept"][0] == 6 and st["empty_rows"] == 2
    assert np.array_equal(out, np.array([0, -2, 2, 3, -2, 0, 2, -4], dtype=np.float32))


def test_exact_cancellation_elects_positive():
    v = np.array([[2, -3, 1, 0], [-2, 3, -1, 0], [0, 0, 4, 0]], dtype=np.float32)
    out, st = tm.ties_merge(v, 1.0)
    # rows 0 and 1: the kept values cancel exactly, s == 0 elects positive, the mean of the positive ones is returned
    assert np.array_equal(out, np.array([2, 3, 2.5, 0], dtype=np.float32))
    assert st["sign_conflict_rows"] == 3 and st["empty_rows"] == 0
    out, _ = tm.ties_merge(v, 1.0, "sum", scaling=0.5, base=np.ones(4, dtype=np.float32))
    assert np.array_equal(out, np.array([2, 2.5, 3.5, 1], dtype=np.float32))


def test_density_one_keeps_everything_and_density_to_zero_keeps_the_maximum():
    g = np.random.default_rng(5)
    v = g.standard_normal((3, 1001)).astype(np.float32)
    _, st = tm.ties_merge(v, 1.0)
    assert np.array_equal(st["thresholds"], np.abs(v).min(axis=1)) and (st["kept"] == 1001).all()
    assert tm.rank_of(1001, 1.0) == 1 and tm.rank_of(1001, 1e-9) == 1001
    _, st = tm.ties_merge(v, 1e-9)
    assert np.array_equal(st["thresholds"], np.abs(v).max(axis=1)) and (st["kept"] == 1).all()


def test_a_threshold_of_the_callers_own_replaces_the_trim():
    v = np.array([[1, 5], [2, -6]], dtype=np.float32)
    out, st = tm.ties_merge(v, 1.0, tau=np.array([[9, 0], [0, 0]], dtype=np.float32))
    assert np.array_equal(out, np.array([2, -6], dtype=np.float32)) and st["kept"].tolist() == [1, 2]
