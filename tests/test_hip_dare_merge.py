"""
GPU tests of the drop-and-rescale (DARE) merge on the dictionaries of a fused run (merge.dare_merge_parameters ->
svdq_plan_dare_merge).  The truth is always tests/dare_model.py applied to what ``reconstruct_task_vectors`` returns on
the same dictionaries (those bits are pinned in test_hip_task_models.py): merged tensors bit for bit, kept counts equal.

Shapes: one row up to 70001 rows (several work units), with every block edge of both rows-per-lane variants: 63 / 64 / 65
(one wave instruction), 127 / 128 / 129 (RB at 17+ tasks), 255 / 256 / 257 (RB up to 16), 513 (2 RB + 1).  Task counts 1,
3, 4, 5, 8, 9, 16, 17, 20, 32: 4 and 5 cross a quad of the generator, 16 and 17 the rows-per-lane change; group padding
(1, 3, 5, 9, 17, 20), one to four task groups.  Every case runs the whole grid of drop rates {0, 0.5, 0.9, 0.99} x rescale
x weights x base.

Non-finite store values are outside the definition (tests/test_hip_ties_merge.py says where the quantizer writes them),
so the stores are built as that file's "k1" profile -- k capped at 1 and one residual stage -- and every store asserts
that what it reconstructs is finite.
"""
import numpy as np
import pytest
import torch

import dare_model as dm

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 13, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 4097, 70001]
NAMES = [f"p{rows:05d}" for rows in ROWS]
SIZES = dict(zip(NAMES, ROWS))
D = sum(ROWS)
LACKING = ("p00257", "p04097")      # the "missing" configuration: one task lacks these two
DROP_RATES = (0.0, 0.5, 0.9, 0.99)
SEED = 0x9E3779B97F4A7C15             # both key words in use


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _tasks(n):
    return [f"t{i:02d}" for i in range(n)]


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _given_weights(T):
    """Non-uniform, of both signs, multiples of 1/8: their sum is exact in double in any order."""
    return [0.125 * (1 + (5 * g) % 7) * (-1 if g % 5 == 3 else 1) for g in range(T)]


_STORES = {}


def _store(sq, T, fp16=True, center=True, missing=False):
    """One fused run per configuration, the values the store reconstructs (v, has [T, D]) and the words of SEED; shared
    and left unchanged."""
    key = (T, fp16, center, missing)
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
                             svd_max_rank=1, svd_rtvq_stages=1)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    shapes = {n: torch.Size([r]) for n, r in SIZES.items()}
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    if missing:
        assert all(n not in recon[lacks] for n in LACKING)
    bad = sorted({n for t in tasks for n, x in recon[t].items() if not bool(torch.isfinite(x).all())})
    assert not bad, f"the store reconstructs non-finite values for {bad}: outside the definition"
    v, has = dm.stack_values(recon, tasks, NAMES, SIZES)
    g = torch.Generator().manual_seed(7 + T)
    base = {n: torch.randn(s, generator=g).cuda() for n, s in shapes.items()}
    _STORES[key] = (cfg, bases, comp, shapes, tasks, v, has, base, dm.words(T, D, SEED))
    return _STORES[key]


def _check(sq, store, v, has, order, words, drop_rate, rescale, weights, normalize, scaling, with_base, seed=SEED, **kw):
    cfg, bases, comp, shapes, _, _, _, base, _ = store
    wd = None if weights is None else dict(zip(order, weights))
    got, stats = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=drop_rate, seed=seed, rescale=rescale,
                                          weights=wd, normalize=normalize, scaling=scaling,
                                          base_state_dict=base if with_base else None, device="cuda", return_stats=True,
                                          **kw)
    base_flat = dm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0][0] if with_base else None
    want, ws = dm.dare_merge(v, has, drop_rate, seed, rescale, weights, normalize, scaling, base_flat, all_words=words)
    what = (len(order), drop_rate, rescale, weights is not None, normalize, scaling, with_base)
    assert sorted(got) == NAMES, what
    want_by = dm.split_rows(want, NAMES, SIZES)
    for n in NAMES:
        assert got[n].is_cuda and got[n].shape == shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    assert list(stats["kept"]) == list(order), what
    assert [stats["kept"][t] for t in order] == ws["kept"].tolist(), what
    assert stats["rows"] == D and stats["drop_threshold"] == ws["drop_threshold"] == dm.drop_threshold(drop_rate), what
    return stats, ws


def _grid(sq, store, v, has, order, words, **kw):
    """Every drop rate x rescale x weights x base.  Returns the model's kept counts per drop rate."""
    kept = {}
    for drop_rate in DROP_RATES:
        for rescale in (True, False):
            for weights in (None, _given_weights(len(order))):
                for with_base in (False, True):
                    scaling = 0.3 if with_base else 1.0
                    _, ws = _check(sq, store, v, has, order, words, drop_rate, rescale, weights, False, scaling,
                                   with_base, **kw)
                    kept[drop_rate] = ws["kept"]
    return kept


CASES = [(T, fp16, center) for T in (1, 3, 4, 5, 8, 9, 16, 17, 20, 32) for fp16 in (True, False)
         for center in (True, False)]


@pytest.mark.parametrize("T,fp16,center", CASES)
def test_merge_matches_the_model_bit_for_bit(sq, T, fp16, center):
    store = _store(sq, T, fp16, center)
    cfg, bases, comp, shapes, tasks, v, has, base, words = store
    plan = bases["p70001"]["masked"]._batch[0].plan
    assert plan.fp16 == fp16 and plan.center == center and plan.N == T
    assert plan.sizes.n_units > plan.P      # a parameter spans more than one work unit
    assert int(bases["p70001"]["masked"]["k"]) == 1
    assert bases["p70001"]["masked"]["U_low"].shape[1] > 0 or T == 1      # both fma chains run
    assert has.all() and np.abs(v).sum(axis=1).all()
    kept = _grid(sq, store, v, has, tasks, words)
    # the draw does something here: nothing is dropped at 0, and about D (1 - p) values survive otherwise
    assert (kept[0.0] == D).all()
    for p in DROP_RATES[1:]:
        assert (np.abs(kept[p] - D * (1 - p)) <= 6 * np.sqrt(D * p * (1 - p))).all(), (p, kept[p])
    # weights divided by their sum on the host, in double
    _check(sq, store, v, has, tasks, words, 0.9, True, [abs(w) for w in _given_weights(T)], True, 0.3, True)


def test_drop_rate_zero_is_task_arithmetic(sq):
    """Unit weights, no draw: the values added task by task -- the sum a user of reconstruct_task_vectors would form."""
    store = _store(sq, 8)
    cfg, bases, comp, shapes, tasks, v, has, base, words = store
    got = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.0, device="cuda")
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    for n in NAMES:
        s = torch.zeros_like(recon[tasks[0]][n])
        for t in tasks:
            s = s + recon[t][n]
        assert torch.equal(got[n].view(torch.int32), s.view(torch.int32)), n


@pytest.mark.parametrize("T,fp16", [(8, True), (20, False)])
def test_a_task_that_lacks_parameters_contributes_nothing_there(sq, T, fp16):
    store = _store(sq, T, fp16, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, words = store
    lacks = min(3, T - 1)
    off = {n: sum(ROWS[:i]) for i, n in enumerate(NAMES)}
    for n in LACKING:
        assert not has[lacks, off[n]:off[n] + SIZES[n]].any() and has[lacks - 1, off[n]:off[n] + SIZES[n]].all()
    plans = {id(bases[n]["masked"]._batch[0].plan) for n in NAMES}
    assert len(plans) == 2      # the two parameters live in a plan of T - 1 tasks: its slot 3 is store task 4, of quad 1
    kept = _grid(sq, store, v, has, tasks, words)
    assert kept[0.0][lacks] == D - sum(SIZES[n] for n in LACKING) and kept[0.0][lacks - 1] == D


def test_a_subset_of_tasks(sq):
    store = _store(sq, 8, True, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, words = store
    pick = [tasks[6], tasks[3], tasks[0]]      # any order in: the merge runs in sorted-name order, g = 0, 1, 2
    rows = [0, 3, 6]
    sub = dm.words(3, D, SEED)
    assert np.array_equal(sub, words[:3])      # the store task index is the index among the MERGED tasks
    _grid(sq, store, v[rows], has[rows], [tasks[i] for i in rows], sub, tasks=pick)
    _check(sq, store, v[[5]], has[[5]], [tasks[5]], dm.words(1, D, 3), 0.5, True, [2.5], False, 1.0, False, seed=3,
           tasks=[tasks[5]])
    with pytest.raises(ValueError, match="nobody"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[0], "nobody"])
    with pytest.raises(ValueError, match="weight of task 't03' is missing"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, tasks=pick, weights={tasks[0]: 1.0, tasks[6]: 1.0})


def test_two_calls_give_identical_bits_and_seeds_differ(sq):
    store = _store(sq, 9, False, True)
    cfg, bases, comp, shapes, tasks, v, has, base, words = store
    kw = dict(drop_rate=0.9, weights=dict(zip(tasks, _given_weights(9))), device="cuda", return_stats=True)
    one, s1 = sq.dare_merge_parameters(comp, bases, shapes, cfg, seed=SEED, **kw)
    two, s2 = sq.dare_merge_parameters(comp, bases, shapes, cfg, seed=SEED, **kw)
    assert s1 == s2
    for n in NAMES:
        assert one[n].data_ptr() != two[n].data_ptr() and torch.equal(one[n].view(torch.int32), two[n].view(torch.int32))
    # the model at other seeds: 0, the largest, and one that differs from SEED in the upper key word only
    for seed in (0, (1 << 64) - 1, SEED ^ (1 << 63)):
        _check(sq, store, v, has, tasks, dm.words(9, D, seed), 0.9, True, None, False, 1.0, False, seed=seed)
    other, s3 = sq.dare_merge_parameters(comp, bases, shapes, cfg, seed=SEED ^ (1 << 63), **kw)
    assert s3["kept"] != s1["kept"] and not torch.equal(other["p70001"], one["p70001"])


def _plan_tables(sq, store):
    """The one plan of a full store with the tables merge.dare_merge_parameters would build for it."""
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    jobs, rows, live = sq.merge._ties_jobs(NAMES, tasks, comp, bases, shapes)
    (batch, entries), = jobs.values()
    plan, T = batch.plan, len(tasks)
    slot_task = np.zeros((plan.P, T), dtype=np.int32)
    task_map = np.full((plan.P, T), -1, dtype=np.int32)
    for i, name in entries.items():
        for j, (g, q) in enumerate(live[name]):
            task_map[i, j], slot_task[i, j] = g, q
    rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * plan.P].view(torch.int64)
    return plan, entries, torch.from_numpy(slot_task).cuda(), torch.from_numpy(task_map).cuda(), rows_dev


def test_plan_level_call_with_rows_past_two_to_the_32(sq):
    """row_base near 2^32: counter word 1 is 0 for the first rows and 1 for the rest, at the shapes of this file."""
    store = _store(sq, 5)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    plan, entries, slot_task, task_map, rows_dev = _plan_tables(sq, store)
    T, row0 = 5, (1 << 32) - 10000
    off = {n: sum(ROWS[:i]) for i, n in enumerate(NAMES)}
    assert off["p70001"] < 10000 < off["p70001"] + 70001      # 2^32 falls inside the largest parameter
    row_base = np.zeros(plan.P, dtype=np.int64)
    out_tab = np.zeros(plan.P, dtype=np.int64)
    outs = {}
    for i, name in entries.items():
        row_base[i] = row0 + off[name]
        outs[name] = torch.empty(SIZES[name], dtype=torch.float32, device="cuda")
        out_tab[i] = outs[name].data_ptr()
    weights = _given_weights(T)
    state = torch.zeros(sq._native.lib().svdq_dare_work_bytes(T) // 8, dtype=torch.int64, device="cuda")
    seed, p = 12345, 0.5
    plan.dare_merge(slot_task, task_map, T, torch.from_numpy(row_base).cuda(), torch.tensor(weights, device="cuda"), state,
                    torch.from_numpy(out_tab).cuda(), seed=seed, drop_threshold=dm.drop_threshold(p),
                    keep_scale=float(dm.keep_scale(p)), scaling=0.5, rows_dev=rows_dev)
    torch.cuda.synchronize()
    want, ws = dm.dare_merge(v, has, p, seed, True, weights, False, 0.5, row0=row0)
    low, _ = dm.dare_merge(v, has, p, seed, True, weights, False, 0.5, row0=0)
    assert not np.array_equal(want, low)      # the global row matters
    for n, x in dm.split_rows(want, NAMES, SIZES).items():
        assert _same_bits(outs[n].cpu().numpy(), x), n
    assert state[:T].tolist() == ws["kept"].tolist()


def test_plan_level_call_validates_its_tables(sq):
    store = _store(sq, 8)
    plan, entries, slot_task, task_map, rows_dev = _plan_tables(sq, store)
    T, P = 8, plan.P
    need = sq._native.lib().svdq_dare_work_bytes(T)
    state = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    outs = torch.full((D,), 7.0, device="cuda")
    out_tab = torch.zeros(P, dtype=torch.int64, device="cuda")
    off = 0
    for i, name in entries.items():
        out_tab[i] = outs.data_ptr() + 4 * off
        off += SIZES[name]
    row_base = torch.zeros(P, dtype=torch.int64, device="cuda")
    w = torch.ones(T, device="cuda")
    who = "svdq_plan_dare_merge"
    bad = [dict(slot_task=slot_task.long()), dict(slot_task=slot_task[:1], task_map=task_map[:1]),
           dict(row_base=row_base.int()), dict(row_base=row_base[:-1]), dict(row_base=row_base.cpu()),
           dict(weights=w.double()), dict(weights=w[:-1]), dict(weights=torch.ones(T + 1, device="cuda")),
           dict(state=state[:T - 1]), dict(state=state.int()), dict(out_table=out_tab[:-1]),
           dict(n_tasks=33), dict(n_tasks=0), dict(seed=-1), dict(seed=1 << 64), dict(drop_threshold=1 << 32),
           dict(drop_threshold=-1)]
    for change in bad:
        args = dict(slot_task=slot_task, task_map=task_map, n_tasks=T, row_base=row_base, weights=w, state=state,
                    out_table=out_tab, seed=1, drop_threshold=1 << 31, keep_scale=0.5)
        args.update(change)
        with pytest.raises(ValueError, match=who):
            plan.dare_merge(rows_dev=rows_dev, **args)
    torch.cuda.synchronize()
    assert not state.any() and bool((outs == 7.0).all())      # nothing was launched
