"""
The numpy model of the Model Breadcrumbs merge (tests/breadcrumbs_model.py) against an independent torch restatement:
sort the magnitudes of every tensor and task, keep ``indices[n_bot : D_p - n_top]``, combine.  The inputs have pairwise
distinct magnitudes per (parameter, task) -- asserted -- so the index rule and the model's threshold rule select the same
values and no case is left out.  Then the hand cases where the two rules differ or an edge is met.
"""
import numpy as np
import pytest
import torch

import breadcrumbs_model as bm

SIZES = [1, 2, 7, 64, 257, 1000]
BOUNDS = np.concatenate([[0], np.cumsum(SIZES)])
PAIRS = [(0.9, 0.01), (0.2, 0.0), (1.0, 0.3), (0.5, 0.5), (0.5, 0.7), (2 / 1000, 0.01)]


def _inputs(T, seed):
    """v [T, D] with pairwise distinct magnitudes per (p, t) and both signs; present [P][T] (one task lacks two tensors)."""
    g = np.random.default_rng(seed)
    D = int(BOUNDS[-1])
    v = np.zeros((T, D), dtype=np.float32)
    for t in range(T):
        for p, n in enumerate(SIZES):
            mags = (g.permutation(n) + 1).astype(np.float32) * np.float32(2.0 ** -7) * np.float32(1 + p)
            v[t, BOUNDS[p]:BOUNDS[p + 1]] = mags * g.choice(np.array([-1, 1], dtype=np.float32), n)
    present = [[not (T > 1 and t == T - 1 and p in (2, 4)) for t in range(T)] for p in range(len(SIZES))]
    for p in range(len(SIZES)):
        for t in range(T):
            m = np.abs(v[t, BOUNDS[p]:BOUNDS[p + 1]])
            assert len(np.unique(m)) == len(m)      # distinct: index rule == threshold rule
    return v, present


def _torch_restatement(v, present, density, gamma, scaling, sign_election, merge_func):
    """float64 sums over the values an argsort-and-slice keeps; thresholds and kept counts from the slice."""
    vt = torch.from_numpy(v)
    T, D = vt.shape
    keep = torch.zeros((T, D), dtype=torch.bool)
    th, kept = {}, {}
    for p, n in enumerate(SIZES):
        n_keep, n_top = int(n * density), int(n * gamma)
        n_bot = n - n_keep - n_top
        if n_bot < 0:
            n_top, n_bot = n_top + n_bot, 0
        for t in range(T):
            if not present[p][t]:
                continue
            seg = vt[t, BOUNDS[p]:BOUNDS[p + 1]]
            idx = torch.argsort(seg.abs())[n_bot:n - n_top] if n_keep > 0 else torch.zeros(0, dtype=torch.long)
            keep[t, BOUNDS[p] + idx] = True
            kept[p, t] = int(idx.numel())
            th[p, t] = (float(seg.abs()[idx[0]]), float(seg.abs()[idx[-1]])) if idx.numel() else None
    x = vt.double() * keep
    if sign_election:
        pos = x.sum(0) >= 0
        agree = keep & torch.where(pos, vt > 0, vt < 0)
    else:
        agree = keep
    a, c = (vt.double() * agree).sum(0), agree.sum(0).double()
    merged = a if merge_func == "sum" else a / c.clamp(min=1)
    return (scaling * merged).numpy(), th, kept, (vt.abs().double() * keep).sum(0).numpy()


@pytest.mark.parametrize("T", [1, 3, 8, 20])
@pytest.mark.parametrize("density,gamma", PAIRS)
def test_model_matches_the_sorted_index_restatement(T, density, gamma):
    v, present = _inputs(T, 100 + T)
    for sign_election in (False, True):
        for merge_func in ("sum", "mean"):
            got, st = bm.breadcrumbs_merge(v, BOUNDS, present, density, gamma, 1.0, sign_election, merge_func)
            want, th, kept, sabs = _torch_restatement(v, present, density, gamma, 1.0, sign_election, merge_func)
            for p in range(len(SIZES)):
                for t in range(T):
                    if not present[p][t]:
                        assert st["thresholds"][p][t] is None and st["kept"][p, t] == 0
                        continue
                    lh = st["thresholds"][p][t]
                    assert (None if lh is None else (float(lh[0]), float(lh[1]))) == th[p, t], (p, t)
                    assert st["kept"][p, t] == kept[p, t], (p, t)
            # the bound of fp32 task-by-task sums against float64 ones.  The values here are small multiples of 2^-7, so
            # every partial sum is exact in both: the elected sign cannot differ, and only the mean's division rounds
            bound = T * 2.0 ** -23 * sabs
            assert (np.abs(got.astype(np.float64) - want) <= bound).all()
            assert st["kept_total"].tolist() == [sum(kept.get((p, t), 0) for p in range(len(SIZES))) for t in range(T)]


def _one(values, density, gamma, **kw):
    """One parameter; values [T][D]."""
    v = np.asarray(values, dtype=np.float32)
    present = kw.pop("present", [[True] * v.shape[0]])
    return bm.breadcrumbs_merge(v, [0, v.shape[1]], present, density, gamma, **kw)


def test_a_tie_at_lo_keeps_every_equal_magnitude():
    # D = 10, density 0.5, gamma 0.2: n_keep 5, n_top 2, n_bot 3 -> lo = 4th smallest, hi = 8th smallest
    out, st = _one([[1, 2, 3, 3, -3, 5, 6, 7, 8, 9]], 0.5, 0.2)
    assert st["thresholds"][0][0] == (3.0, 7.0) and st["kept"][0, 0] == 6      # three 3s, not one
    assert out.tolist() == [0, 0, 3, 3, -3, 5, 6, 7, 0, 0]


def test_a_tie_at_hi_keeps_every_equal_magnitude():
    out, st = _one([[1, 2, 3, 4, 5, 6, 7, -7, 7, 9]], 0.5, 0.2)
    assert st["thresholds"][0][0] == (4.0, 7.0) and st["kept"][0, 0] == 6      # n_keep is 5
    assert out.tolist() == [0, 0, 0, 4, 5, 6, 7, -7, 7, 0]


def test_lo_equal_to_hi():
    # D = 10, density 0.1, gamma 0.3: n_keep 1, n_top 3, n_bot 6 -> lo = hi = the 7th smallest
    out, st = _one([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], 0.1, 0.3)
    assert st["thresholds"][0][0] == (7.0, 7.0) and st["kept"][0, 0] == 1
    assert out.tolist() == [0, 0, 0, 0, 0, 0, 7, 0, 0, 0]


def test_all_magnitudes_equal_keeps_everything():
    out, st = _one([[2, -2, 2, -2, 2, 2, -2, 2]], 0.25, 0.25)
    assert st["thresholds"][0][0] == (2.0, 2.0) and st["kept"][0, 0] == 8 and st["empty_rows"] == 0


def test_a_negative_n_bot_clamps_n_top():
    # D = 10, density 0.5, gamma 0.7: n_keep 5, n_top 7 -> n_bot -2 -> n_top 5, n_bot 0: the density is met
    assert bm.counts(10, 0.5, 0.7) == (5, 5, 0)
    out, st = _one([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], 0.5, 0.7)
    assert st["thresholds"][0][0] == (1.0, 5.0) and st["kept"][0, 0] == 5
    # density 1 keeps everything, whatever gamma is
    assert bm.counts(10, 1.0, 0.3) == (10, 0, 0)
    out, st = _one([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10]], 1.0, 0.3)
    assert st["kept"][0, 0] == 10


def test_n_keep_zero_keeps_nothing():
    out, st = _one([[1, 2, 3, 4]], 0.2, 0.0, base=np.ones(4, dtype=np.float32))
    assert st["thresholds"][0][0] is None and st["kept"][0, 0] == 0 and st["empty_rows"] == 4
    assert out.tolist() == [1, 1, 1, 1]


def test_a_single_row():
    out, st = _one([[-3.0]], 1.0, 0.5)
    assert st["thresholds"][0][0] == (3.0, 3.0) and out.tolist() == [-3.0]
    out, st = _one([[-3.0]], 0.9, 0.0)
    assert st["thresholds"][0][0] is None and out.tolist() == [0.0]


def test_a_task_that_lacks_a_parameter_contributes_nothing():
    v = np.array([[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60]], dtype=np.float32)
    present = [[True, True], [True, False]]      # task 1 lacks the second parameter (rows 3 .. 5)
    out, st = bm.breadcrumbs_merge(v, [0, 3, 6], present, 1.0, 0.0, merge_func="mean")
    assert out.tolist() == [5.5, 11, 16.5, 4, 5, 6]
    assert st["thresholds"][1][1] is None and st["kept"].tolist() == [[3, 3], [3, 0]]
    assert st["kept_total"].tolist() == [6, 3]


def test_election_and_both_merge_functions():
    # row 0: 3 - 2 elects positive; row 1: 1 - 1 = 0 elects positive (s == 0); row 2: both negative
    v = [[3, 1, -1], [-2, -1, -2]]
    out, st = _one(v, 1.0, 0.0, sign_election=True, merge_func="sum")
    assert out.tolist() == [3, 1, -3] and st["sign_conflict_rows"] == 2
    out, _ = _one(v, 1.0, 0.0, sign_election=True, merge_func="mean")
    assert out.tolist() == [3, 1, -1.5]
    out, _ = _one(v, 1.0, 0.0, sign_election=False, merge_func="mean", scaling=2.0)
    assert out.tolist() == [1, 0, -3]
