"""
GPU tests of the sign-elected (TIES) merge on the dictionaries of a fused run (merge.ties_merge_parameters ->
svdq_plan_ties_hist / svdq_ties_select_step / svdq_plan_ties_merge).  The truth is always tests/ties_model.py applied to
what ``reconstruct_task_vectors`` returns on the same dictionaries (those bits are pinned in test_hip_task_models.py):
merged tensors and thresholds bit for bit, kept counts and both row counters equal.

Shapes: the ragged set of test_hip_adopt.py (one row up to 70001 rows: several work units).  Task counts 1, 3, 8, 9, 16,
17, 20, 32: group padding (1, 3, 9, 17, 20), both rows-per-lane variants (<= 16, > 16), one to four task groups.

Non-finite store values are outside the definition, and the coefficient quantizer writes them where its input has no
range: a low part of one coefficient, or of two coefficients at the second residual stage (scale = inf, 0 / 0 on the way
back) -- which the three-row parameter and every parameter of a three-task run have under the usual settings.  So the
stores here come in two profiles, and every store asserts that what it reconstructs is finite:
    "plain"  energy threshold 0.9, no rank cap, two residual stages (finite at 1 and 8 tasks)
    "k1"     k capped at 1 and one residual stage: a one-column U_high chain, every other direction in U_low
"""
import numpy as np
import pytest
import torch

import ties_model as tm

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 13, 255, 256, 257, 4095, 4096, 4097, 8193, 70001]
NAMES = [f"p{rows:05d}" for rows in ROWS]
SIZES = dict(zip(NAMES, ROWS))
D = sum(ROWS)
LACKING = ("p00257", "p04097")      # the "missing" configuration: one task lacks these two
DENSITIES = (0.2, 1.0, 3.0 / D)


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _tasks(n):
    return [f"t{i:02d}" for i in range(n)]


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_STORES = {}


PROFILES = {"plain": dict(svd_max_rank=None, svd_rtvq_stages=2), "k1": dict(svd_max_rank=1, svd_rtvq_stages=1)}


def _store(sq, T, fp16=True, center=True, missing=False, profile="k1"):
    """One fused run per configuration and the values the store reconstructs, v [T, D]; shared and left unchanged."""
    key = (T, fp16, center, missing, profile)
    if key in _STORES:
        return _STORES[key]
    from oracle import svd_hybrid_oracle as orc
    tasks = _tasks(T)
    tv = {t: {} for t in tasks}
    for rows in ROWS:
        for t, d in zip(tasks, orc.synthetic_deltas(rows, T, 31 * T + rows, rank=3)):
            tv[t][f"p{rows:05d}"] = d.cuda()
    lacks = tasks[min(3, T - 1)]
    if missing:
        for name in LACKING:
            del tv[lacks][name]
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_low_bits=4, svd_fp16=fp16, svd_center=center,
                             **PROFILES[profile])
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    shapes = {n: torch.Size([r]) for n, r in SIZES.items()}
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    if missing:
        assert all(n not in recon[lacks] for n in LACKING)
    v = tm.stack_values(recon, tasks, NAMES, SIZES)
    bad = sorted({n for t in tasks for n, x in recon[t].items() if not bool(torch.isfinite(x).all())})
    assert not bad, f"the store reconstructs non-finite values for {bad}: outside the definition"
    g = torch.Generator().manual_seed(7 + T)
    base = {n: torch.randn(s, generator=g).cuda() for n, s in shapes.items()}
    _STORES[key] = (cfg, bases, comp, shapes, tasks, v, base)
    return _STORES[key]


def _check(sq, store, v, order, density, merge_func, scaling, with_base, **kw):
    cfg, bases, comp, shapes, _, _, base = store
    got, stats = sq.ties_merge_parameters(comp, bases, shapes, cfg, density=density, scaling=scaling, merge_func=merge_func,
                                          base_state_dict=base if with_base else None, device="cuda", return_stats=True,
                                          **kw)
    base_flat = tm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0] if with_base else None
    want, ws = tm.ties_merge(v, density, merge_func, scaling, base_flat)
    what = (len(order), density, merge_func, scaling, with_base)
    assert sorted(got) == NAMES, what
    want_by = tm.split_rows(want, NAMES, SIZES)
    for n in NAMES:
        assert got[n].is_cuda and got[n].shape == shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    assert list(stats["thresholds"]) == list(order) and list(stats["kept"]) == list(order), what
    tau = np.array([stats["thresholds"][t] for t in order], dtype=np.float32)
    assert _same_bits(tau, ws["thresholds"]), (what, tau, ws["thresholds"])
    assert [stats["kept"][t] for t in order] == ws["kept"].tolist(), what
    assert stats["sign_conflict_rows"] == ws["sign_conflict_rows"] and stats["empty_rows"] == ws["empty_rows"], what
    assert stats["rows"] == D
    return stats, ws


CASES = [(T, True, True, "k1") for T in (3, 8, 9, 16, 17, 20, 32)] + \
        [(1, True, True, "plain"), (8, True, True, "plain"), (8, False, True, "plain"), (8, True, False, "plain"),
         (3, False, False, "k1"), (17, False, True, "k1"), (20, True, False, "k1"), (32, False, False, "k1")]


@pytest.mark.parametrize("T,fp16,center,profile", CASES)
def test_merge_matches_the_model_bit_for_bit(sq, T, fp16, center, profile):
    store = _store(sq, T, fp16, center, profile=profile)
    cfg, bases, comp, shapes, tasks, v, base = store
    plan = bases["p70001"]["masked"]._batch[0].plan
    assert plan.fp16 == fp16 and plan.center == center and plan.N == T
    assert plan.sizes.n_units > plan.P      # a parameter spans more than one work unit
    k = int(bases["p70001"]["masked"]["k"])
    assert bases["p70001"]["masked"]["U_low"].shape[1] > 0 or T == 1      # both fma chains run
    assert k == 1 if profile == "k1" else k >= 1
    for density in DENSITIES:
        for merge_func in ("mean", "sum"):
            for with_base in (False, True):
                scaling = 0.3 if (with_base or merge_func == "sum") else 1.0
                stats, ws = _check(sq, store, v, tasks, density, merge_func, scaling, with_base)
                keep_n = int(D * density)
                assert all(c >= max(keep_n, 1) for c in ws["kept"])
    # the trim does something here: at density 0.2 most rows lose values, and signs do conflict among the kept ones
    _, ws = tm.ties_merge(v, 0.2)
    if T > 1:
        assert ws["sign_conflict_rows"] > 0
    assert (ws["kept"] < D).all()


@pytest.mark.parametrize("T,fp16", [(8, True), (20, False)])
def test_a_task_that_lacks_parameters_ranks_their_rows_as_zeros(sq, T, fp16):
    store = _store(sq, T, fp16, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, base = store
    lacks = min(3, T - 1)
    off = {n: sum(ROWS[:i]) for i, n in enumerate(NAMES)}
    for n in LACKING:
        assert not v[lacks, off[n]:off[n] + SIZES[n]].any() and v[lacks - 1, off[n]:off[n] + SIZES[n]].any()
    plans = {id(bases[n]["masked"]._batch[0].plan) for n in NAMES}
    assert len(plans) == 2      # the two parameters live in a plan of T - 1 tasks: the thresholds span both plans
    for density in DENSITIES:
        for merge_func, with_base in (("mean", True), ("sum", False)):
            stats, ws = _check(sq, store, v, tasks, density, merge_func, 0.3, with_base)
    # density 1: tau of the lacking task is 0 -- its implicit zeros are kept and counted
    stats, ws = _check(sq, store, v, tasks, 1.0, "mean", 1.0, False)
    assert stats["thresholds"][tasks[lacks]] == 0.0 and stats["kept"][tasks[lacks]] == D and stats["empty_rows"] == 0


def test_a_subset_of_tasks(sq):
    store = _store(sq, 8, True, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, base = store
    pick = [tasks[6], tasks[3], tasks[0]]      # any order in: the merge runs in sorted-name order
    rows = [0, 3, 6]
    for density, merge_func in ((0.2, "mean"), (1.0, "sum")):
        _check(sq, store, v[rows], [tasks[i] for i in rows], density, merge_func, 0.3, True, tasks=pick)
    _check(sq, store, v[[5]], [tasks[5]], 0.2, "mean", 1.0, False, tasks=[tasks[5]])
    with pytest.raises(ValueError, match="nobody"):
        sq.ties_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[0], "nobody"])


def test_plan_level_calls_validate_their_tables(sq):
    store = _store(sq, 8)
    plan = store[1]["p70001"]["masked"]._batch[0].plan
    state = sq.TiesState(8, plan.device)
    ok = torch.zeros((plan.P, 8), dtype=torch.int32, device=plan.device)
    with pytest.raises(ValueError, match="svdq_plan_ties_hist"):
        plan.ties_hist(ok.long(), ok, 8, 0, state.table)
    with pytest.raises(ValueError, match="svdq_plan_ties_hist"):
        plan.ties_hist(ok[:1], ok[:1], 8, 0, state.table)
    with pytest.raises(ValueError, match="digit"):
        plan.ties_hist(ok, ok, 8, 4, state.table)
    with pytest.raises(ValueError, match="n_tasks"):
        plan.ties_hist(ok, ok, 33, 0, state.table)
    with pytest.raises(ValueError, match="merge_func"):
        plan.ties_merge(ok, ok, 8, state.table, torch.zeros(plan.P, dtype=torch.int64, device=plan.device), "max")
    with pytest.raises(ValueError, match="n_tasks"):
        sq.TiesState(0, plan.device)
    torch.cuda.synchronize()
    assert not state.table.any()      # nothing was launched
