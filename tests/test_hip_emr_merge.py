"""
GPU tests of the EMR merge on the dictionaries of a fused run (merge.emr_merge_parameters -> svdq_plan_emr_elect,
merge.emr_task_state_dict -> svdq_emr_apply).  The truth is always tests/emr_model.py applied to what
``reconstruct_task_vectors`` returns on the same dictionaries (those bits are pinned in test_hip_task_models.py): tau_uni
bit for bit (the sign of zero included: uint32 views), every task's packed stream byte for byte, every task model bit for
bit.

The two sums per task are fp64 sums of n non-negative terms in the kernel's own fixed order; the model adds them exactly
(math.fsum).  Any order of fp64 addition of n non-negative terms errs by at most (n - 1) 2^-53 relative to first order, so
the bound is n 2^-52 relative, n the rows the task has -- derived, not measured; the factor 2 covers the higher-order term.

The stores are built as tests/test_hip_tall_consensus.py builds its own (its shapes and its plan-table helper are
imported): parameters of 1 .. 70001 rows with every block edge of both rows-per-lane variants and of the 32-bit stream
word, later parameters at unaligned bit offsets, 1 .. 32 tasks (every task-group and rows-per-lane dispatch), fp16 and
fp32 bases, centred or not.  The generator's seeds are that file's plus an offset: with its own seeds task 2 of 8 agrees
with the elected sign on all 64 rows of p00064 -- a full mask, which the conditions below (asserted on the model alone)
do not accept as a test of the mask bits.  With three or four tasks of this generator one task outweighs the others on
most rows, so few seeds leave every 64-row parameter both kinds of bits for every task; the offsets of those two counts
were picked with the model alone, on the generator's deltas on the CPU, for the most rows to spare (11 and 7).
"""
import numpy as np
import pytest
import torch

import emr_model as em
import tall_model as tm
import test_hip_tall_consensus as ttc

pytestmark = pytest.mark.gpu

ROWS, NAMES, SIZES, D, OFF, LACKING, N_BYTES = ttc.ROWS, ttc.NAMES, ttc.SIZES, ttc.D, ttc.OFF, ttc.LACKING, ttc.N_BYTES
REL = 2.0 ** -52


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


SEED = {3: 20000, 4: 11000}      # by task count; 2000 for every other
_STORES, _MODELS = {}, {}


def _store(sq, T, fp16=True, center=True, missing=False):
    """One fused run per configuration and the values the store reconstructs (v, has [T, D]); shared and left unchanged.
    The tuple is the one test_hip_tall_consensus._store returns."""
    key = (T, fp16, center, missing)
    if key in _STORES:
        return _STORES[key]
    from oracle import svd_hybrid_oracle as orc
    tasks = ttc._tasks(T)
    tv = {t: {} for t in tasks}
    for rows in ROWS:
        for t, d in zip(tasks, orc.synthetic_deltas(rows, T, SEED.get(T, 2000) + 31 * T + rows, rank=3)):
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


def _case(sq, T, fp16=True, center=True, missing=False):
    """(store, model) of one configuration; the model runs once per configuration and is left unchanged."""
    key = (T, fp16, center, missing)
    store = _store(sq, T, fp16, center, missing)
    if key not in _MODELS:
        _MODELS[key] = em.emr_merge(store[5], store[6])
    return store, _MODELS[key]


def _close(got, want, n, what):
    print(f"{what}: got {got!r}, exact {want!r}, relative error {abs(got - want) / want if want else 0.0:.3e}, "
          f"bound {n * REL:.3e}")
    assert abs(got - want) <= n * REL * want, what


def _compare(got, model, order, has, bit_base=OFF, total=D, what=""):
    """The four results of one emr_merge_parameters call against the model."""
    unified, masks, rescalers, stats = got
    assert sorted(unified) == NAMES, what
    for n, x in tm.split_rows(model["tau"], NAMES, SIZES).items():
        assert unified[n].is_cuda and unified[n].dtype is torch.float32 and tuple(unified[n].shape) == (SIZES[n],), (what, n)
        assert np.array_equal(_u32(unified[n].cpu().numpy()), _u32(x)), (what, n)
    streams = tm.pack_streams(tm.split_rows(model["masks"], NAMES, SIZES), bit_base, total)
    assert list(masks) == list(order) == list(rescalers), what
    for g, t in enumerate(order):
        assert masks[t].is_cuda and masks[t].dtype is torch.uint8 and masks[t].shape == ((total + 7) // 8,), (what, t)
        assert np.array_equal(masks[t].cpu().numpy(), streams[g]), (what, t)
    assert stats["rows"] == D and list(stats["active"]) == list(order), what
    assert [stats["active"][t] for t in order] == model["masks"].sum(axis=1).tolist(), what
    for g, t in enumerate(order):
        n = int(has[g].sum())
        _close(stats["abs_sum"][t], float(model["A"][g]), n, f"{what} A[{t}]")
        _close(stats["masked_sum"][t], float(model["B"][g]), n, f"{what} B[{t}]")
        a, b = stats["abs_sum"][t], stats["masked_sum"][t]
        assert rescalers[t] == (a / b if b != 0.0 else 1.0), (what, t)      # the fp64 quotient of the two sums
        assert abs(rescalers[t] - model["lambda"][g]) <= 3 * n * REL * model["lambda"][g], (what, t)


def _assert_not_vacuous(model, v, has, T):
    """Conditions on the model's output alone: the comparison cannot pass on empty or full masks, on an election that is
    a plain maximum of magnitudes, or on rescalers that are all one number."""
    if T < 3:
        return
    top = np.where(has, np.abs(v), 0).max(axis=0)
    problems = []
    for n in NAMES:
        if SIZES[n] < 64:
            continue
        rows = slice(OFF[n], OFF[n] + SIZES[n])
        for g in range(T):
            if has[g, rows].all() and not (model["masks"][g, rows].any() and not model["masks"][g, rows].all()):
                problems.append(f"{n}: the mask of task {g} is {'full' if model['masks'][g, rows].all() else 'empty'}")
        if not (np.abs(model["tau"][rows]) < top[rows]).any():      # the largest magnitude disagreed somewhere
            problems.append(f"{n}: every row elects its largest magnitude")
    if len(set(model["lambda"].tolist())) <= 1:
        problems.append("the rescalers are all equal")
    assert not problems, problems


CASES = [(T, fp16, center) for T in (1, 3, 4, 8, 9, 16, 17, 32) for fp16 in (True, False) for center in (True, False)]


@pytest.mark.parametrize("T,fp16,center", CASES)
def test_elected_vector_masks_and_sums_match_the_model(sq, T, fp16, center):
    store, model = _case(sq, T, fp16, center)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    plan = bases["p70001"]["masked"]._batch[0].plan
    assert plan.fp16 == fp16 and plan.center == center and plan.N == T
    assert plan.sizes.n_units > plan.P      # a parameter spans more than one work unit
    assert has.all()
    _assert_not_vacuous(model, v, has, T)
    got = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    _compare(got, model, tasks, has, what=f"T = {T}, fp16 {fp16}, centred {center}")
    if T == 1:      # the task's own vector, mask v != 0, rescaler exactly 1
        assert np.array_equal(model["masks"][0], v[0] != 0) and got[2][tasks[0]] == 1.0
        assert np.array_equal(model["tau"], np.where(v[0] != 0, v[0], np.float32(0)))
    plain = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda")
    assert len(plain) == 3 and plain[2] == got[2]


@pytest.mark.parametrize("T,fp16", [(8, True), (20, False)])
def test_a_task_that_lacks_parameters_has_zero_bits_there(sq, T, fp16):
    store, model = _case(sq, T, fp16, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    lacks = min(3, T - 1)
    for n in LACKING:
        assert not has[lacks, OFF[n]:OFF[n] + SIZES[n]].any() and has[lacks - 1, OFF[n]:OFF[n] + SIZES[n]].all()
    assert len({id(bases[n]["masked"]._batch[0].plan) for n in NAMES}) == 2      # two plans share the state
    _assert_not_vacuous(model, v, has, T)
    got = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    _compare(got, model, tasks, has, what=f"T = {T}, one task lacks two parameters")
    bits = np.unpackbits(got[1][tasks[lacks]].cpu().numpy())[:D]
    for n in LACKING:
        assert not bits[OFF[n]:OFF[n] + SIZES[n]].any()
        assert model["masks"][lacks - 1, OFF[n]:OFF[n] + SIZES[n]].any()      # its neighbour's bits there are set
    # A of the lacking task holds none of those rows: it is the sum over the rows it has
    full = float(np.abs(v[lacks]).astype(np.float64).sum())
    assert got[3]["abs_sum"][tasks[lacks]] <= full and int(has[lacks].sum()) == D - sum(SIZES[n] for n in LACKING)


def test_a_subset_of_tasks(sq):
    store, _ = _case(sq, 8, True, True, missing=True)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    pick = [tasks[6], tasks[3], tasks[0]]      # any order in: the merge runs in sorted-name order, g = 0, 1, 2
    rows = [0, 3, 6]
    model = em.emr_merge(v[rows], has[rows])
    got = sq.emr_merge_parameters(comp, bases, shapes, cfg, tasks=pick, device="cuda", return_stats=True)
    _compare(got, model, [tasks[i] for i in rows], has[rows], what="subset")
    one = sq.emr_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[5]], device="cuda", return_stats=True)
    _compare(one, em.emr_merge(v[[5]], has[[5]]), [tasks[5]], has[[5]], what="one task of eight")
    with pytest.raises(ValueError, match="nobody"):
        sq.emr_merge_parameters(comp, bases, shapes, cfg, tasks=[tasks[0], "nobody"])


def test_a_reference_with_extra_keys_shifts_the_bits(sq):
    store, model = _case(sq, 9, False, True)
    cfg, bases, comp, shapes, tasks, v, has, base, base_flat = store
    ref = {n: torch.empty(SIZES[n], device="meta") for n in NAMES}
    ref.update({"a.first": torch.empty(7, 3, device="meta"), "p00100.between": torch.empty(45, device="meta"),
                "p04097.between": torch.empty(1, device="meta"), "z.last": torch.empty(19, device="meta"),
                "p00002.removed": torch.empty(11, device="meta")})
    keys = sorted(k for k in ref if k != "p00002.removed")
    bit_base, total = {}, 0
    for key in keys:
        bit_base[key] = total
        total += ref[key].numel()
    assert total == D + 21 + 45 + 1 + 19
    got = sq.emr_merge_parameters(comp, bases, shapes, cfg, reference_state_dict=ref, remove_keys=["p00002.removed"],
                                  device="cuda", return_stats=True)
    _compare(got, model, tasks, has, bit_base, total, what="shifted")
    plain = tm.pack_streams(tm.split_rows(model["masks"], NAMES, SIZES), OFF, D)
    for g, t in enumerate(tasks):
        host = got[1][t].cpu().numpy()
        assert not np.array_equal(host[:N_BYTES], plain[g])      # the bits did move
        bits = np.unpackbits(host)[:total]
        for key in ("a.first", "p00100.between", "p04097.between", "z.last"):
            assert not bits[bit_base[key]:bit_base[key] + ref[key].numel()].any()
    # the task model reads the shifted streams with the same layout
    t = tasks[4]
    out = sq.emr_task_state_dict(got[0], got[1], got[2], t, base_state_dict=base, reference_state_dict=ref,
                                 remove_keys=["p00002.removed"], device="cuda")
    want = em.task_model(model["tau"], model["masks"][4], got[2][t], base_flat)
    for n, x in tm.split_rows(want, NAMES, SIZES).items():
        assert np.array_equal(_u32(out[n].cpu().numpy()), _u32(x)), n
    with pytest.raises(ValueError, match="'p00013' of the store has no place in the mask streams"):
        sq.emr_merge_parameters(comp, bases, shapes, cfg, reference_state_dict=ref, remove_keys=["p00013"], device="cuda")
    short = dict(ref, p00513=torch.empty(512, device="meta"))
    with pytest.raises(ValueError, match=r"reference_state_dict\['p00513'\] has 512 elements, the store holds 513 rows"):
        sq.emr_merge_parameters(comp, bases, shapes, cfg, reference_state_dict=short, device="cuda")


def test_two_calls_give_identical_bits_the_sums_included(sq):
    store, _ = _case(sq, 9, False, True)
    cfg, bases, comp, shapes, tasks = store[:5]
    u1, m1, r1, s1 = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    u2, m2, r2, s2 = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    as_int = lambda d: np.array([d[t] for t in tasks], dtype=np.float64).view(np.int64).tolist()      # noqa: E731
    assert as_int(s1["abs_sum"]) == as_int(s2["abs_sum"]) and as_int(s1["masked_sum"]) == as_int(s2["masked_sum"])
    assert as_int(r1) == as_int(r2) and s1["active"] == s2["active"]
    for n in NAMES:
        assert u1[n].data_ptr() != u2[n].data_ptr() and torch.equal(u1[n].view(torch.int32), u2[n].view(torch.int32))
    for t in tasks:
        assert m1[t].data_ptr() != m2[t].data_ptr() and torch.equal(m1[t], m2[t])


GUARD = 64


def _state(sq, T):
    return torch.zeros(sq._native.lib().svdq_emr_state_bytes(T) // 8, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("lead", [0, 37])
def test_plan_level_call_leaves_the_guard_bytes_alone(sq, lead):
    """Streams and tau_uni buffers with 64 guard bytes either side, filled with 0xA5, at a caller's own bit offsets
    (``lead`` bits before the first parameter); tau_uni NULL for two parameters: their bits and sums are written all the
    same.  Called twice: the second call leaves the same bits, the sums in its own state included."""
    T = 5
    store, model = _case(sq, T)
    cfg, bases, comp, shapes, tasks, v, has, base, _ = store
    plan, entries, slot_task, task_map, rows_dev = ttc._plan_tables(sq, store)
    total = lead + D
    n_words = (total + 31) // 32
    buf = torch.full((T, GUARD + 4 * n_words + GUARD), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:, GUARD:GUARD + 4 * n_words] = 0
    assert buf.data_ptr() % 4 == 0 and buf.shape[1] % 4 == 0
    mask_tab = torch.tensor([buf[g].data_ptr() + GUARD for g in range(T)], dtype=torch.int64, device="cuda")
    # one buffer for every tau_uni, guard bytes between the parameters: [GUARD | rows[p] floats | GUARD] ...
    skipped = ("p00033", "p70001")
    at, where = 0, {}
    for n in NAMES:
        where[n] = at + GUARD
        at += GUARD + 4 * SIZES[n] + GUARD
    uni = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
    bit_base = np.zeros(plan.P, dtype=np.int64)
    uni_tab = np.zeros(plan.P, dtype=np.int64)
    for i, name in entries.items():
        bit_base[i] = lead + OFF[name]
        if name not in skipped:
            uni_tab[i] = uni.data_ptr() + where[name]
    state = _state(sq, T)
    args = (slot_task, task_map, T, torch.from_numpy(bit_base).cuda(), torch.from_numpy(uni_tab).cuda(), mask_tab, state)
    plan.emr_elect(*args, rows_dev=rows_dev)
    torch.cuda.synchronize()
    once = state.clone()
    streams = tm.pack_streams(tm.split_rows(model["masks"], NAMES, SIZES), {n: lead + OFF[n] for n in NAMES}, total)
    host = buf.cpu().numpy()
    assert (host[:, :GUARD] == 0xA5).all() and (host[:, GUARD + 4 * n_words:] == 0xA5).all()
    n_bytes = (total + 7) // 8
    for g in range(T):
        assert np.array_equal(host[g, GUARD:GUARD + n_bytes], streams[g]), g
        assert not host[g, GUARD + n_bytes:GUARD + 4 * n_words].any()      # the rest of the last word
    flat = uni.cpu().numpy()
    for n, x in tm.split_rows(model["tau"], NAMES, SIZES).items():
        lo, hi = where[n], where[n] + 4 * SIZES[n]
        assert (flat[lo - GUARD:lo] == 0xA5).all() and (flat[hi:hi + GUARD] == 0xA5).all(), n
        if n in skipped:
            assert (flat[lo:hi] == 0xA5).all(), n
        else:
            assert np.array_equal(flat[lo:hi].view(np.uint32), _u32(x)), n
    for g in range(T):
        _close(float(once[g]), float(model["A"][g]), D, f"plan level A[{g}]")
        _close(float(once[T + g]), float(model["B"][g]), D, f"plan level B[{g}]")
    assert not once[2 * T:].any()
    # a second call on the same streams and a fresh state: the bits are OR'ed or stored again, the sums the same bits
    again = _state(sq, T)
    plan.emr_elect(*args[:-1], again, rows_dev=rows_dev)
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int64), once.view(torch.int64))
    assert np.array_equal(buf.cpu().numpy(), host) and np.array_equal(uni.cpu().numpy(), flat)


def test_plan_level_call_validates_its_arguments(sq):
    T = 8
    store, _ = _case(sq, T)
    plan, entries, slot_task, task_map, rows_dev = ttc._plan_tables(sq, store)
    P = plan.P
    state = _state(sq, T)
    outs = torch.full((D,), 7.0, device="cuda")
    streams = torch.zeros((T, (D + 31) // 32), dtype=torch.int32, device="cuda")
    uni_tab = torch.zeros(P, dtype=torch.int64, device="cuda")
    bit_base = torch.zeros(P, dtype=torch.int64, device="cuda")
    for i, name in entries.items():
        uni_tab[i] = outs.data_ptr() + 4 * OFF[name]
        bit_base[i] = OFF[name]
    mask_tab = torch.tensor([streams[g].data_ptr() for g in range(T)], dtype=torch.int64, device="cuda")
    who = "svdq_plan_emr_elect"
    bad = [dict(slot_task=slot_task.long()), dict(slot_task=slot_task[:1], task_map=task_map[:1]),
           dict(bit_base=bit_base.int()), dict(bit_base=bit_base[:-1]), dict(bit_base=bit_base.cpu()),
           dict(state=state[:2 * T - 1]), dict(state=state.float()), dict(state=state.view(torch.int64)),
           dict(uni_table=uni_tab[:-1]), dict(uni_table=None), dict(mask_table=mask_tab[:-1]),
           dict(mask_table=mask_tab.int()), dict(mask_table=None), dict(n_tasks=33), dict(n_tasks=0)]
    for change in bad:
        args = dict(slot_task=slot_task, task_map=task_map, n_tasks=T, bit_base=bit_base, uni_table=uni_tab,
                    mask_table=mask_tab, state=state)
        args.update(change)
        with pytest.raises(ValueError, match=who):
            plan.emr_elect(rows_dev=rows_dev, **args)
    # the entry point's own refusals (SVDQ_EINVAL with a message), with the real plan
    lib, EINVAL, nat = sq._native.lib(), sq._native.SVDQ_EINVAL, sq._native
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    need = lib.svdq_emr_work_bytes(plan._h, T, T)
    assert need == lib.svdq_task_reconstruct_work_bytes(plan._h, T) + -(-plan.sizes.n_units * 2 * T * 8 // 256) * 256
    assert lib.svdq_emr_work_bytes(plan._h, 0, T) == 0 and lib.svdq_emr_work_bytes(plan._h, T, 33) == 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(bits=bit_base, u=uni_tab, m=mask_tab, s=state, w=work, n_tasks=T, mean=plan.mean):
        return lib.svdq_plan_emr_elect(plan._h, ptr(rows_dev), ptr(plan.small), ptr(plan.basis), ptr(mean),
                                       ptr(slot_task), ptr(task_map), T, n_tasks, ptr(bits), ptr(u), ptr(m), ptr(s), ptr(w),
                                       None)
    for kw, word in ((dict(bits=None), "bit_base"), (dict(u=None), "uni_ptrs"), (dict(m=None), "mask_ptrs"),
                     (dict(s=None), "state"), (dict(w=None), "work"), (dict(n_tasks=0), "n_tasks"),
                     (dict(n_tasks=33), "n_tasks"), (dict(mean=None), "mean")):
        assert call(**kw) == EINVAL, kw
        assert who in nat.last_error() and word in nat.last_error(), (kw, nat.last_error())
    torch.cuda.synchronize()
    assert not state.any() and bool((outs == 7.0).all()) and not streams.any()      # nothing was launched


# ---------------------------------------------------------------------------------------------------- the task model
@pytest.mark.parametrize("T,fp16", [(8, True), (17, False)])
def test_every_task_model_matches_the_model_bit_for_bit(sq, T, fp16):
    store, model = _case(sq, T, fp16, True)
    cfg, bases, comp, shapes, tasks, v, has, base, base_flat = store
    unified, masks, rescalers = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda")
    half = dict(base, p04097=base["p04097"].half())      # a base that is not fp32: added afterwards, in torch's arithmetic
    half_flat = base_flat.copy()
    half_flat[OFF["p04097"]:OFF["p04097"] + 4097] = half["p04097"].float().cpu().numpy()
    for g, t in enumerate(tasks):
        lam = rescalers[t]
        for b, flat in ((None, None), (base, base_flat)) + (((half, half_flat),) if g == 2 else ()):
            out = sq.emr_task_state_dict(unified, masks, rescalers, t, base_state_dict=b, device="cuda")
            want = em.task_model(model["tau"], model["masks"][g], lam, flat)
            assert sorted(out) == NAMES
            for n, x in tm.split_rows(want, NAMES, SIZES).items():
                assert out[n].is_cuda and out[n].dtype is torch.float32 and out[n].shape == unified[n].shape, (t, n)
                assert np.array_equal(_u32(out[n].cpu().numpy()), _u32(x)), (t, n, b is not None)
    # the scalar overridden, a negative one among the values: -lambda * +0 is -0
    for lam in (0.5, -1.25, 0.0):
        out = sq.emr_task_state_dict(unified, masks, rescalers, tasks[1], rescale=lam, device="cuda")
        want = em.task_model(model["tau"], model["masks"][1], lam)
        for n, x in tm.split_rows(want, NAMES, SIZES).items():
            assert np.array_equal(_u32(out[n].cpu().numpy()), _u32(x)), (lam, n)
    # from host tensors, to host tensors
    host = sq.emr_task_state_dict({n: x.cpu() for n, x in unified.items()}, {t: m.cpu() for t, m in masks.items()},
                                  rescalers, tasks[0], base_state_dict={n: x.cpu() for n, x in base.items()}, device="cpu")
    want = em.task_model(model["tau"], model["masks"][0], rescalers[tasks[0]], base_flat)
    for n, x in tm.split_rows(want, NAMES, SIZES).items():
        assert not host[n].is_cuda and np.array_equal(_u32(host[n].numpy()), _u32(x)), n


@pytest.mark.parametrize("lead", [0, 37])
def test_plan_level_apply_with_out_aliasing_base(sq, lead):
    """svdq_emr_apply on the caller's own tables: every parameter inside ONE flat buffer that is base and output at
    once, at offsets that are no multiple of 16 bytes (the 4-byte path) after 16-byte aligned ones (the 16-byte path),
    guard bytes around it; a NULL output skips its parameter."""
    T = 8
    store, model = _case(sq, T)
    cfg, bases, comp, shapes, tasks, v, has, base, base_flat = store
    unified, masks, rescalers = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda")
    g = 5
    total = lead + D
    words = torch.zeros((total + 31) // 32 * 4, dtype=torch.uint8, device="cuda")
    packed = tm.pack_streams(tm.split_rows(model["masks"][[g]], NAMES, SIZES), {n: lead + OFF[n] for n in NAMES}, total)[0]
    words[:packed.size] = torch.from_numpy(packed).cuda()
    pad = GUARD // 4
    flat = torch.full((pad + D + pad,), 123.0, device="cuda")
    flat[pad:pad + D] = torch.from_numpy(base_flat).cuda()
    uni_flat = torch.from_numpy(model["tau"]).cuda()
    P = len(NAMES)
    rows = torch.tensor([SIZES[n] for n in NAMES], dtype=torch.int64, device="cuda")
    bits = torch.tensor([lead + OFF[n] for n in NAMES], dtype=torch.int64, device="cuda")
    uni_tab = torch.tensor([uni_flat.data_ptr() + 4 * OFF[n] for n in NAMES], dtype=torch.int64, device="cuda")
    skipped = "p00129"
    io = [0 if n == skipped else flat.data_ptr() + 4 * (pad + OFF[n]) for n in NAMES]
    io_tab = torch.tensor(io, dtype=torch.int64, device="cuda")
    assert sum(a % 16 != 0 for a in io if a) >= 8 and any(a % 16 == 0 for a in io if a)
    lam = float(np.float32(rescalers[tasks[g]]))
    lib = sq._native.lib()
    rc = lib.svdq_emr_apply(P, rows.data_ptr(), bits.data_ptr(), uni_tab.data_ptr(), words.data_ptr(), lam,
                            io_tab.data_ptr(), io_tab.data_ptr(), None)
    assert rc == 0, sq._native.last_error()
    torch.cuda.synchronize()
    want = em.task_model(model["tau"], model["masks"][g], lam, base_flat)
    lo, hi = OFF[skipped], OFF[skipped] + SIZES[skipped]
    want[lo:hi] = base_flat[lo:hi]      # untouched
    host = flat.cpu().numpy()
    assert (host[:pad] == 123.0).all() and (host[pad + D:] == 123.0).all()
    assert np.array_equal(_u32(host[pad:pad + D]), _u32(want))
