"""
GPU tests of the TALL masks and the consensus merge on the dictionaries of a fused run (merge.consensus_merge_parameters /
merge.tall_masks_from_store -> svdq_plan_tall_consensus).  The truth is always tests/tall_model.py applied to what
``reconstruct_task_vectors`` returns on the same dictionaries (those bits are pinned in test_hip_task_models.py): merged
tensors bit for bit, every task's packed stream byte for byte, the active and agreement counts equal.

Shapes: one row up to 70001 rows (several work units), with every block edge of both rows-per-lane variants and of the
32-bit stream word: 31 / 32 / 33, 63 / 64 / 65 (one ballot), 127 / 128 / 129 (RB at 17+ tasks), 255 / 256 / 257 (RB up to
16), 513 (2 RB + 1).  The parameters follow each other in the streams without padding, so the odd sizes put every later
parameter at a bit offset that is no multiple of 32 (asserted below).  Task counts 1, 3, 4, 8, 9, 16, 17, 32: one to
four task groups, group padding (3, 9, 17), the rows-per-lane change between 16 and 17.  Every case runs lambda {0, a
middle value, per-task values} x k {0, 1, 2, T} x base.

The middle lambda is min(0.4, 1 / sqrt(T - 1)): 0.4 is the paper's mid-range, and with T tasks of similar scale the sum
of the others grows like sqrt(T - 1) times one task's value, so the lambda at which about half of the values pass shrinks
likewise.  Whether it is a middle value for a store is asserted on the model alone (every task's density inside 5 % ..
95 %, three or more agreement bins in use from 8 tasks on): the comparison with the kernel cannot pass on empty or full
masks.  At T = 1 the mask is v != 0 by definition (the others' sum is 0), so that density is asserted to be 1.

Non-finite store values are outside the definition (tests/test_hip_ties_merge.py says where the quantizer writes them),
so the stores are built as tests/test_hip_dare_merge.py builds them -- k capped at 1 and one residual stage -- and every
store asserts that what it reconstructs is finite.
"""
import math

import numpy as np
import pytest
import torch

import tall_model as tm

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 13, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 4097, 70001]
NAMES = [f"p{rows:05d}" for rows in ROWS]
SIZES = dict(zip(NAMES, ROWS))
D = sum(ROWS)
OFF = {n: sum(ROWS[:i]) for i, n in enumerate(NAMES)}
LACKING = ("p00257", "p04097")      # the "missing" configuration: one task lacks these two
N_BYTES = (D + 7) // 8


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _tasks(n):
    return [f"t{i:02d}" for i in range(n)]


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _middle(T):
    return min(0.4, 1.0 / math.sqrt(max(T - 1, 1)))


def _per_task(T):
    """Per-task lambdas around the middle value, 0 among them from three tasks on."""
    return [_middle(T) * (0.0, 0.5, 1.0, 1.5, 2.5)[(g + 1) % 5] for g in range(T)]


_STORES = {}


def _store(sq, T, fp16=True, center=True, missing=False):
    """One fused run per configuration and the values the store reconstructs (v, has [T, D]); shared and left unchanged."""
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
    v, has = tm.stack_values(recon, tasks, NAMES, SIZES)
    g = torch.Generator().manual_seed(7 + T)
    base = {n: torch.randn(s, generator=g).cuda() for n, s in shapes.items()}
    base_flat = tm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0][0]
    _STORES[key] = (cfg, bases, comp, shapes, tasks, v, has, base, base_flat)
    return _STORES[key]


def _check(sq, store, v, has, order, lam, k, scaling, with_base, **kw):
    """One combined call (merge + masks + stats) against the model.  ``lam``: a number or one per task of ``order``."""
    cfg, bases, comp, shapes, _, _, _, base, base_flat = store
    arg = dict(zip(order, lam)) if isinstance(lam, list) else lam
    got, masks, stats = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=arg, k=k, scaling=scaling,
                                                      base_state_dict=base if with_base else None, return_masks=True,
                                                      device="cuda", return_stats=True, **kw)
    want, wm, ws = tm.consensus_merge(v, has, lam, k, scaling, base_flat if with_base else None)
    what = (len(order), lam if not isinstance(lam, list) else "per task", k, scaling, with_base)
    assert sorted(got) == NAMES, what
    want_by = tm.split_rows(want, NAMES, SIZES)
    for n in NAMES:
        assert got[n].is_cuda and got[n].shape == shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    streams = tm.pack_streams(tm.split_rows(wm, NAMES, SIZES), OFF, D)
    assert list(masks) == list(order), what
    for g, t in enumerate(order):
        assert masks[t].is_cuda and masks[t].dtype is torch.uint8 and masks[t].shape == (N_BYTES,), (what, t)
        assert np.array_equal(masks[t].cpu().numpy(), streams[g]), (what, t)
    assert list(stats["active"]) == list(order), what
    assert [stats["active"][t] for t in order] == ws["active"].tolist(), what
    assert stats["agreement"] == ws["agreement"].tolist() and sum(stats["agreement"]) == D, what
    assert stats["rows"] == D == ws["rows"], what
    return masks, wm, ws


def _grid(sq, store, v, has, order, **kw):
    """lambda {0, middle, per task} x k {0, 1, 2, T} x base / no base (scaling 0.3 / 1.0).  Returns the model's masks and
    statistics at the middle lambda."""
    T = len(order)
    mid = None
    for lam in (0.0, _middle(T), _per_task(T)):
        for k in sorted({0, 1, min(2, T), T}):
            for with_base in (False, True):
                _, wm, ws = _check(sq, store, v, has, order, lam, k, 0.3 if with_base else 1.0, with_base, **kw)
                if lam == _middle(T):
                    mid = (wm, ws)
    return mid


def _assert_not_vacuous(wm, ws, has, T):
    """The condition on the model alone: the middle lambda gives masks that are neither empty nor full."""
    density = wm.sum(axis=1) / has.sum(axis=1)
    print(f"T = {T}: middle lambda {_middle(T):.4f}, density {density.min():.3f} .. {density.max():.3f}, agreement bins "
          f"in use {(ws['agreement'] > 0).sum()} of {T + 1}")
    if T == 1:
        assert density[0] == 1.0      # v != 0: the others' sum is 0
        return
    assert (density > 0.05).all() and (density < 0.95).all(), density
    if T >= 8:
        assert (ws["agreement"] > 0).sum() >= 3, ws["agreement"]


def test_later_parameters_sit_at_unaligned_bit_offsets():
    assert sum(OFF[n] % 32 != 0 for n in NAMES) >= 12 and OFF["p70001"] % 32 != 0 and OFF["p04097"] % 8 != 0
    assert D % 8 != 0 and (D + 31) // 32 * 4 > N_BYTES      # the last word of a stream is partial, its last byte too


CASES = [(T, fp16, center) for T in (1, 3, 4, 8, 9, 16, 17, 32) for fp16 in (True, False) for center in (True, False)]


@pytest.mark.parametrize("T,fp16,center", CASES)
def test_merge_and_masks_match_the_model_bit_for_bit(sq, T, fp16, center):
    store = _store(sq, T, fp16, center)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    plan = bases["p70001"]["masked"]._batch[0].plan
    assert plan.fp16 == fp16 and plan.center == center and plan.N == T
    assert plan.sizes.n_units > plan.P      # a parameter spans more than one work unit
    assert int(bases["p70001"]["masked"]["k"]) == 1
    assert bases["p70001"]["masked"]["U_low"].shape[1] > 0 or T == 1      # both fma chains run
    assert has.all() and np.abs(v).sum(axis=1).all()
    wm, ws = _grid(sq, store, v, has, tasks)
    _assert_not_vacuous(wm, ws, has, T)


def test_k_zero_is_task_arithmetic_and_lambda_zero_marks_the_non_zero_values(sq):
    store = _store(sq, 8)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    got, masks = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=0.0, k=0, return_masks=True,
                                               device="cuda")
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    for n in NAMES:
        s = torch.zeros_like(recon[tasks[0]][n])
        for t in tasks:
            s = s + recon[t][n]
        assert torch.equal(got[n].view(torch.int32), s.view(torch.int32)), n
    for g, t in enumerate(tasks):
        bits = np.unpackbits(masks[t].cpu().numpy())[:D].astype(bool)
        assert np.array_equal(bits, v[g] != 0), t


@pytest.mark.parametrize("T,fp16", [(8, True), (20, False)])
def test_a_task_that_lacks_parameters_has_zero_bits_there(sq, T, fp16):
    store = _store(sq, T, fp16, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    lacks = min(3, T - 1)
    for n in LACKING:
        assert not has[lacks, OFF[n]:OFF[n] + SIZES[n]].any() and has[lacks - 1, OFF[n]:OFF[n] + SIZES[n]].all()
    plans = {id(bases[n]["masked"]._batch[0].plan) for n in NAMES}
    assert len(plans) == 2      # the two parameters live in a plan of T - 1 tasks: its slot 3 is store task 4
    wm, ws = _grid(sq, store, v, has, tasks)
    _assert_not_vacuous(wm, ws, has, T)
    masks, wm0, _ = _check(sq, store, v, has, tasks, 0.0, 1, 1.0, False)
    bits = np.unpackbits(masks[tasks[lacks]].cpu().numpy())[:D]
    for n in LACKING:
        assert not bits[OFF[n]:OFF[n] + SIZES[n]].any()
        assert wm0[lacks - 1, OFF[n]:OFF[n] + SIZES[n]].any()      # its neighbour's bits there are set
    # every row of the two parameters counts at most T - 1 masks: the agreement bin T holds rows of the others only
    assert ws["agreement"].sum() == D


def test_a_subset_of_tasks(sq):
    store = _store(sq, 8, True, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    pick = [tasks[6], tasks[3], tasks[0]]      # any order in: the merge runs in sorted-name order, g = 0, 1, 2
    rows = [0, 3, 6]
    _grid(sq, store, v[rows], has[rows], [tasks[i] for i in rows], tasks=pick)
    _check(sq, store, v[[5]], has[[5]], [tasks[5]], 0.4, 1, 1.0, False, tasks=[tasks[5]])
    with pytest.raises(ValueError, match="nobody"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[0], "nobody"])
    with pytest.raises(ValueError, match="k must be an integer in \\[0, 3\\]"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tasks=pick, k=4)
    with pytest.raises(ValueError, match="tall_lambda of task 't03' is missing"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tasks=pick, tall_lambda={tasks[0]: 1.0, tasks[6]: 1.0})


def test_a_reference_with_extra_keys_shifts_the_bits(sq):
    """Keys that sort before, between and after the store's parameters: the store's bits move, the extra keys' bits are 0,
    and remove_keys takes a key out of the layout."""
    store = _store(sq, 9, False, True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    ref = {n: torch.empty(SIZES[n], device="meta") for n in NAMES}
    ref.update({"a.first": torch.empty(7, 3, device="meta"), "p00100.between": torch.empty(45, device="meta"),
                "p04097.between": torch.empty(1, device="meta"), "z.last": torch.empty(19, device="meta"),
                "p00002.removed": torch.empty(11, device="meta")})
    keys = sorted(k for k in ref if k != "p00002.removed")
    assert keys[0] == "a.first" and keys[-1] == "z.last" and keys.index("p00100.between") == keys.index("p00127") - 1
    bit_base, total = {}, 0
    for key in keys:
        bit_base[key] = total
        total += ref[key].numel()
    assert total == D + 21 + 45 + 1 + 19
    lam, k = _middle(9), 2
    got, masks, stats = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=lam, k=k,
                                                      reference_state_dict=ref, remove_keys=["p00002.removed"],
                                                      return_masks=True, device="cuda", return_stats=True)
    want, wm, ws = tm.consensus_merge(v, has, lam, k)
    streams = tm.pack_streams(tm.split_rows(wm, NAMES, SIZES), bit_base, total)
    plain = tm.pack_streams(tm.split_rows(wm, NAMES, SIZES), OFF, D)
    for g, t in enumerate(tasks):
        assert masks[t].shape == ((total + 7) // 8,) and np.array_equal(masks[t].cpu().numpy(), streams[g]), t
        assert not np.array_equal(streams[g][:N_BYTES], plain[g])      # the bits did move
        bits = np.unpackbits(streams[g])[:total]
        for key in ("a.first", "p00100.between", "p04097.between", "z.last"):
            assert not bits[bit_base[key]:bit_base[key] + ref[key].numel()].any()
    assert stats["agreement"] == ws["agreement"].tolist()
    for n, x in tm.split_rows(want, NAMES, SIZES).items():
        assert _same_bits(got[n].cpu().numpy(), x), n
    # through the package's own unpacking: the per-parameter masks come back under their names
    host_ref = {key: torch.zeros(x.shape) for key, x in ref.items()}
    per = sq.vector_to_state_dict(torch.from_numpy(np.unpackbits(masks[tasks[4]].cpu().numpy())[:total].copy()), host_ref,
                                  ["p00002.removed"])
    for n, x in tm.split_rows(wm[4], NAMES, SIZES).items():
        assert np.array_equal(per[n].numpy().astype(bool), x), n
    # refusals: a store parameter without a place, or with another element count
    with pytest.raises(ValueError, match="'p00013' of the store has no place in the mask streams"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, reference_state_dict=ref, remove_keys=["p00013"],
                                      return_masks=True, device="cuda")
    short = dict(ref, p00513=torch.empty(512, device="meta"))
    with pytest.raises(ValueError, match=r"reference_state_dict\['p00513'\] has 512 elements, the store holds 513 rows"):
        sq.tall_masks_from_store(comp, bases, shapes, cfg, reference_state_dict=short, device="cuda")


def test_mask_only_and_merge_only_calls_give_the_bits_of_the_combined_call(sq):
    store = _store(sq, 17, True, False)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    lam, k = _per_task(17), 2
    arg = dict(zip(tasks, lam))
    both, masks, stats = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=arg, k=k, scaling=0.3,
                                                       base_state_dict=base, return_masks=True, device="cuda",
                                                       return_stats=True)
    only_m, stats_m = sq.tall_masks_from_store(comp, bases, shapes, cfg, tall_lambda=arg, device="cuda", return_stats=True)
    only_o, stats_o = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=arg, k=k, scaling=0.3,
                                                    base_state_dict=base, device="cuda", return_stats=True)
    assert stats == stats_m == stats_o
    for t in tasks:
        assert torch.equal(masks[t], only_m[t]) and masks[t].data_ptr() != only_m[t].data_ptr(), t
    for n in NAMES:
        assert torch.equal(both[n].view(torch.int32), only_o[n].view(torch.int32)), n
    assert any(bool(m.any()) for m in masks.values())


def test_two_calls_give_identical_bits(sq):
    store = _store(sq, 9, False, True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    kw = dict(tall_lambda=_middle(9), k=3, return_masks=True, device="cuda", return_stats=True)
    one, m1, s1 = sq.consensus_merge_parameters(comp, bases, shapes, cfg, **kw)
    two, m2, s2 = sq.consensus_merge_parameters(comp, bases, shapes, cfg, **kw)
    assert s1 == s2
    for n in NAMES:
        assert one[n].data_ptr() != two[n].data_ptr() and torch.equal(one[n].view(torch.int32), two[n].view(torch.int32))
    for t in tasks:
        assert m1[t].data_ptr() != m2[t].data_ptr() and torch.equal(m1[t], m2[t])


def _plan_tables(sq, store):
    """The one plan of a full store with the tables merge.consensus_merge_parameters would build for it."""
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


GUARD = 64


@pytest.mark.parametrize("lead", [0, 37])
def test_plan_level_call_leaves_the_guard_bytes_alone(sq, lead):
    """Streams with 64 guard bytes either side, filled with 0xA5, at a caller's own bit offsets (``lead`` bits before the
    first parameter); outputs NULL for two parameters: their bits are written all the same."""
    store = _store(sq, 5)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    plan, entries, slot_task, task_map, rows_dev = _plan_tables(sq, store)
    T = 5
    total = lead + D
    n_words = (total + 31) // 32
    buf = torch.full((T, GUARD + 4 * n_words + GUARD), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:, GUARD:GUARD + 4 * n_words] = 0
    assert buf.data_ptr() % 4 == 0 and buf.shape[1] % 4 == 0
    mask_tab = torch.tensor([buf[g].data_ptr() + GUARD for g in range(T)], dtype=torch.int64, device="cuda")
    bit_base = np.zeros(plan.P, dtype=np.int64)
    out_tab = np.zeros(plan.P, dtype=np.int64)
    outs = {}
    skipped = ("p00033", "p70001")
    for i, name in entries.items():
        bit_base[i] = lead + OFF[name]
        if name not in skipped:
            outs[name] = torch.empty(SIZES[name], dtype=torch.float32, device="cuda")
            out_tab[i] = outs[name].data_ptr()
    lam = _per_task(T)
    state = torch.zeros(sq._native.lib().svdq_tall_work_bytes(T) // 8, dtype=torch.int64, device="cuda")
    plan.tall_consensus(slot_task, task_map, T, torch.from_numpy(bit_base).cuda(),
                        torch.tensor(lam, dtype=torch.float32, device="cuda"), state,
                        out_table=torch.from_numpy(out_tab).cuda(), mask_table=mask_tab, min_agree=2, scaling=0.5,
                        rows_dev=rows_dev)
    torch.cuda.synchronize()
    want, wm, ws = tm.consensus_merge(v, has, lam, 2, 0.5)
    streams = tm.pack_streams(tm.split_rows(wm, NAMES, SIZES), {n: lead + OFF[n] for n in NAMES}, total)
    host = buf.cpu().numpy()
    assert (host[:, :GUARD] == 0xA5).all() and (host[:, GUARD + 4 * n_words:] == 0xA5).all()
    n_bytes = (total + 7) // 8
    for g in range(T):
        assert np.array_equal(host[g, GUARD:GUARD + n_bytes], streams[g]), g
        assert not host[g, GUARD + n_bytes:GUARD + 4 * n_words].any()      # the rest of the last word
    for n, x in tm.split_rows(want, NAMES, SIZES).items():
        if n not in skipped:
            assert _same_bits(outs[n].cpu().numpy(), x), n
    assert state[:T].tolist() == ws["active"].tolist() and state[T:2 * T + 1].tolist() == ws["agreement"].tolist()


def test_plan_level_call_validates_its_arguments(sq):
    store = _store(sq, 8)
    plan, entries, slot_task, task_map, rows_dev = _plan_tables(sq, store)
    T, P = 8, plan.P
    need = sq._native.lib().svdq_tall_work_bytes(T)
    state = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    outs = torch.full((D,), 7.0, device="cuda")
    streams = torch.zeros((T, (D + 31) // 32), dtype=torch.int32, device="cuda")
    out_tab = torch.zeros(P, dtype=torch.int64, device="cuda")
    bit_base = torch.zeros(P, dtype=torch.int64, device="cuda")
    for i, name in entries.items():
        out_tab[i] = outs.data_ptr() + 4 * OFF[name]
        bit_base[i] = OFF[name]
    mask_tab = torch.tensor([streams[g].data_ptr() for g in range(T)], dtype=torch.int64, device="cuda")
    lam = torch.full((T,), 0.4, device="cuda")
    who = "svdq_plan_tall_consensus"
    bad = [dict(slot_task=slot_task.long()), dict(slot_task=slot_task[:1], task_map=task_map[:1]),
           dict(bit_base=bit_base.int()), dict(bit_base=bit_base[:-1]), dict(bit_base=bit_base.cpu()),
           dict(lambdas=lam.double()), dict(lambdas=lam[:-1]), dict(lambdas=torch.ones(T + 1, device="cuda")),
           dict(state=state[:2 * T]), dict(state=state.int()), dict(out_table=out_tab[:-1]),
           dict(mask_table=mask_tab[:-1]), dict(mask_table=mask_tab.int()), dict(out_table=None, mask_table=None),
           dict(n_tasks=33), dict(n_tasks=0), dict(min_agree=-1), dict(min_agree=T + 1), dict(min_agree=2.0),
           dict(min_agree=True)]
    for change in bad:
        args = dict(slot_task=slot_task, task_map=task_map, n_tasks=T, bit_base=bit_base, lambdas=lam, state=state,
                    out_table=out_tab, mask_table=mask_tab, min_agree=2)
        args.update(change)
        with pytest.raises(ValueError, match=who):
            plan.tall_consensus(rows_dev=rows_dev, **args)
    # the entry point's own refusals (SVDQ_EINVAL with a message), with the real plan: both outputs NULL, k out of range,
    # a missing table
    lib, EINVAL, nat = sq._native.lib(), sq._native.SVDQ_EINVAL, sq._native
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    plan._ties_tables(who, slot_task, task_map)

    def call(bits=bit_base, lams=lam, k=2, o=out_tab, m=mask_tab, n_tasks=T):
        return lib.svdq_plan_tall_consensus(plan._h, ptr(rows_dev), ptr(plan.small), ptr(plan.basis), ptr(plan.mean),
                                            ptr(slot_task), ptr(task_map), T, n_tasks, ptr(bits), ptr(lams), k, 1.0, None,
                                            ptr(o), ptr(m), ptr(state), ptr(plan._task_work), None)
    for kw, word in ((dict(o=None, m=None), "both NULL"), (dict(k=-1), "min_agree"), (dict(k=T + 1), "min_agree"),
                     (dict(bits=None), "bit_base"), (dict(lams=None), "lambdas"), (dict(n_tasks=0), "n_tasks")):
        assert call(**kw) == EINVAL, kw
        assert who in nat.last_error() and word in nat.last_error(), (kw, nat.last_error())
    torch.cuda.synchronize()
    assert not state.any() and bool((outs == 7.0).all()) and not streams.any()      # nothing was launched
