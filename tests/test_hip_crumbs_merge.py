"""
GPU tests of the Model Breadcrumbs merge on the dictionaries of a fused run (merge.breadcrumbs_merge_parameters ->
svdq_plan_crumbs_hist / svdq_plan_crumbs_select_step / svdq_plan_crumbs_merge).  The truth is always
tests/breadcrumbs_model.py applied to what ``reconstruct_task_vectors`` returns on the same dictionaries: merged tensors
and both thresholds of every (parameter, task) bit for bit, kept counts and both row counters equal.

The stores are those of tests/test_hip_ties_merge.py (its ragged shapes, its two profiles, its case list; every store
asserts that it reconstructs finite values) -- built once and shared with that file where both run.
"""
import numpy as np
import pytest
import torch

import breadcrumbs_model as bm
import test_hip_ties_merge as ttm
import ties_model as tm

pytestmark = pytest.mark.gpu

ROWS, NAMES, SIZES, D, LACKING, CASES = ttm.ROWS, ttm.NAMES, ttm.SIZES, ttm.D, ttm.LACKING, ttm.CASES
BOUNDS = np.concatenate([[0], np.cumsum(ROWS)])
# the defaults | the per-tensor TIES trim | everything kept | n_bot exactly 0 on even sizes | the clamp | n_keep 2 on
# the largest tensor and 0 on every other
PAIRS = ((0.9, 0.01), (0.2, 0.0), (1.0, 0.3), (0.5, 0.5), (0.5, 0.7), (2 / 70001, 0.01))


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _bits(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _present(tasks, order, missing):
    lacks = tasks[min(3, len(tasks) - 1)]
    return [[not (missing and n in LACKING and t == lacks) for t in order] for n in NAMES]


def _check(sq, store, v, order, present, density, gamma, sign_election, merge_func, scaling, with_base, banded=None, **kw):
    cfg, bases, comp, shapes, _, _, base = store
    got, stats = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, density=density, gamma=gamma, scaling=scaling,
                                                 sign_election=sign_election, merge_func=merge_func,
                                                 base_state_dict=base if with_base else None, device="cuda",
                                                 return_stats=True, **kw)
    base_flat = tm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0] if with_base else None
    want, ws = bm.breadcrumbs_merge(v, BOUNDS, present, density, gamma, scaling, sign_election, merge_func, base_flat,
                                    banded=banded)
    what = (len(order), density, gamma, sign_election, merge_func, scaling, with_base)
    assert sorted(got) == NAMES, what
    want_by = tm.split_rows(want, NAMES, SIZES)
    for p, n in enumerate(NAMES):
        assert got[n].is_cuda and got[n].shape == shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert ttm._same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
        have = [t for g, t in enumerate(order) if present[p][g]]
        assert list(stats["thresholds"][n]) == have and list(stats["kept"][n]) == have, (what, n)
        for g, t in enumerate(order):
            if not present[p][g]:
                continue
            lh, wlh = stats["thresholds"][n][t], ws["thresholds"][p][g]
            assert (lh is None) == (wlh is None), (what, n, t)
            if lh is not None:
                assert _bits(lh).tolist() == _bits(wlh).tolist(), (what, n, t, lh, wlh)
            assert stats["kept"][n][t] == ws["kept"][p, g], (what, n, t)
    assert [stats["kept_total"][t] for t in order] == ws["kept_total"].tolist(), what
    assert stats["sign_conflict_rows"] == ws["sign_conflict_rows"] and stats["empty_rows"] == ws["empty_rows"], what
    assert stats["rows"] == D
    return got, stats, ws


def _all_ways(sq, store, v, order, present, pairs=PAIRS, **kw):
    """Every pair with election on and off, both merge functions, with and without base; the model's band once a pair."""
    seen = {}
    for density, gamma in pairs:
        banded = bm.bands(v, BOUNDS, present, density, gamma)
        for sign_election in (False, True):
            for merge_func in ("sum", "mean"):
                for with_base in (False, True):
                    scaling = 0.3 if (with_base or merge_func == "sum") else 1.0
                    _, _, ws = _check(sq, store, v, order, present, density, gamma, sign_election, merge_func, scaling,
                                      with_base, banded=banded, **kw)
        seen[density, gamma] = ws
    return seen


@pytest.mark.parametrize("T,fp16,center,profile", CASES)
def test_merge_matches_the_model_bit_for_bit(sq, T, fp16, center, profile):
    store = ttm._store(sq, T, fp16, center, profile=profile)
    cfg, bases, comp, shapes, tasks, v, base = store
    plan = bases["p70001"]["masked"]._batch[0].plan
    assert plan.fp16 == fp16 and plan.center == center and plan.N == T
    assert plan.sizes.n_units > plan.P      # a parameter spans more than one work unit
    k = int(bases["p70001"]["masked"]["k"])
    assert bases["p70001"]["masked"]["U_low"].shape[1] > 0 or T == 1      # both fma chains run
    assert k == 1 if profile == "k1" else k >= 1
    seen = _all_ways(sq, store, v, tasks, _present(tasks, tasks, False))
    for (density, gamma), ws in seen.items():
        for p, rows in enumerate(ROWS):
            n_keep, n_top, n_bot = bm.counts(rows, density, gamma)
            assert (ws["kept"][p] >= n_keep).all()
            if n_keep == 0:
                assert not ws["kept"][p].any()
    # the cases do what they are named for
    assert (seen[1.0, 0.3]["kept"] == np.array(ROWS)[:, None]).all() and seen[1.0, 0.3]["empty_rows"] == 0
    assert bm.counts(4096, 0.5, 0.5) == (2048, 2048, 0) and bm.counts(4096, 0.5, 0.7) == (2048, 2048, 0)
    tiny = seen[2 / 70001, 0.01]["kept"]
    assert (tiny[:-1] == 0).all() and (tiny[-1] >= 2).all() and bm.counts(70001, 2 / 70001, 0.01)[0] == 2
    assert seen[0.9, 0.01]["kept"][-1].max() < 70001      # the outlier cut removes values of the largest tensor
    if T > 1:
        assert seen[0.9, 0.01]["sign_conflict_rows"] > 0


@pytest.mark.parametrize("T,fp16", [(8, True), (20, False)])
def test_a_task_that_lacks_parameters_contributes_nothing_to_them(sq, T, fp16):
    store = ttm._store(sq, T, fp16, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, base = store
    plans = {id(bases[n]["masked"]._batch[0].plan) for n in NAMES}
    assert len(plans) == 2      # the two parameters live in a plan of T - 1 tasks: one state table per plan
    present = _present(tasks, tasks, True)
    seen = _all_ways(sq, store, v, tasks, present)
    lacks = min(3, T - 1)
    for n in LACKING:
        assert seen[1.0, 0.3]["kept"][NAMES.index(n), lacks] == 0
        assert seen[1.0, 0.3]["thresholds"][NAMES.index(n)][lacks] is None


def test_a_subset_of_tasks(sq):
    store = ttm._store(sq, 8, True, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, base = store
    pick = [tasks[6], tasks[3], tasks[0]]      # any order in: the merge runs in sorted-name order
    rows = [0, 3, 6]
    order = [tasks[i] for i in rows]
    present = [[not (n in LACKING and t == tasks[3]) for t in order] for n in NAMES]
    _all_ways(sq, store, v[rows], order, present, pairs=PAIRS[:2], tasks=pick)
    one = [[True] for _ in NAMES]
    _check(sq, store, v[[5]], [tasks[5]], one, 0.9, 0.01, True, "mean", 1.0, False, tasks=[tasks[5]])
    with pytest.raises(ValueError, match="nobody"):
        sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[0], "nobody"])


@pytest.mark.parametrize("T", [8, 20])
def test_two_calls_give_identical_bits(sq, T):
    cfg, bases, comp, shapes, tasks, v, base = ttm._store(sq, T)
    runs = [sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, sign_election=True, merge_func="mean",
                                            base_state_dict=base, return_stats=True) for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    for n in NAMES:
        assert torch.equal(runs[0][0][n].view(torch.int32), runs[1][0][n].view(torch.int32)), n


def test_plan_level_calls_validate_their_arguments(sq):
    store = ttm._store(sq, 20)
    plan = store[1]["p70001"]["masked"]._batch[0].plan
    state = sq.CrumbsState(plan.P, 20, plan.device)
    ok = torch.zeros((plan.P, 20), dtype=torch.int32, device=plan.device)
    ranks = torch.zeros((plan.P, 2), dtype=torch.int64, device=plan.device)
    outs = torch.zeros(plan.P, dtype=torch.int64, device=plan.device)
    with pytest.raises(ValueError, match="svdq_plan_crumbs_hist"):
        plan.crumbs_hist(ok.long(), ok, 20, 0, 1, state.table)
    for digit in (-1, 4):
        with pytest.raises(ValueError, match="svdq_plan_crumbs_hist: digit"):
            plan.crumbs_hist(ok, ok, 20, digit, 1, state.table)
        with pytest.raises(ValueError, match="svdq_plan_crumbs_select_step: digit"):
            plan.crumbs_select(20, digit, ranks, state.table)
    for bounds in (0, 4, -1):
        with pytest.raises(ValueError, match="svdq_plan_crumbs_hist: bounds"):
            plan.crumbs_hist(ok, ok, 20, 0, bounds, state.table)
    with pytest.raises(ValueError, match="bounds 3"):      # both histograms of 20 slots do not fit the LDS
        plan.crumbs_hist(ok, ok, 20, 0, 3, state.table)
    with pytest.raises(ValueError, match="n_tasks"):
        plan.crumbs_hist(ok, ok, 33, 0, 1, state.table)
    with pytest.raises(ValueError, match="state"):      # a table sized for fewer tasks
        plan.crumbs_hist(ok, ok, 20, 0, 1, sq.CrumbsState(plan.P, 8, plan.device).table)
    with pytest.raises(ValueError, match="ranks"):
        plan.crumbs_select(20, 0, ranks[:1], state.table)
    with pytest.raises(ValueError, match="merge_func"):
        plan.crumbs_merge(ok, ok, 20, state.table, outs, merge_func="max")
    with pytest.raises(ValueError, match="out_table"):
        plan.crumbs_merge(ok, ok, 20, state.table, outs[:1])
    with pytest.raises(ValueError, match="n_tasks"):
        sq.CrumbsState(plan.P, 0, plan.device)
    torch.cuda.synchronize()
    assert not state.table.any()      # nothing was launched
