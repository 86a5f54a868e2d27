"""
GPU tests of artifact adoption (include/svdq.h, svdq_plan_import; CompressPlan.import_artifacts;
driver.adopt_artifacts): stored artifacts -- save_all_artifacts -> load_all_artifacts, tensors on the CPU or the GPU --
go into plans byte for byte, the copy launch writes nothing but the three ranges of a parameter, and every merge over
the adopted dictionaries is, bit for bit, the merge over the dictionaries of the fused run that produced the artifacts.

Shapes: the smallest at which a unit, a block or a tail can go wrong -- one row, fewer rows than tasks, around the
256-row block, around the 4096- / 8192-row units, several units with an odd tail -- as ONE ragged parameter set per
configuration; task counts on both sides of the 16-task unit-size switch and at the limit.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 13, 255, 256, 257, 4095, 4096, 4097, 8193, 70001]
TASK_COUNTS = [1, 3, 8, 17, 32]

# name -> (N, config overrides, parameters a task lacks)
CONFIGS = {}
for _n in TASK_COUNTS:
    for _fp16 in (True, False):
        for _center in (True, False):
            CONFIGS[f"n{_n}-{'fp16' if _fp16 else 'fp32'}-{'center' if _center else 'nocenter'}"] = (
                _n, dict(svd_fp16=_fp16, svd_center=_center), ())
CONFIGS["energy1"] = (8, dict(svd_energy_threshold=1.0), ())            # k = r: some U_low are [rows, 0]
CONFIGS["maxrank1"] = (8, dict(svd_max_rank=1), ())
CONFIGS["bits2and8"] = (8, dict(svd_low_bits_by_param=lambda name: 8 if int(name[1:]) % 2 else 2), ())
CONFIGS["stages1"] = (8, dict(svd_rtvq_stages=1), ())
CONFIGS["stages4"] = (8, dict(svd_rtvq_stages=4), ())
CONFIGS["missing"] = (8, {}, ("p00257", "p04097"))                       # a task lacks two parameters: two plans


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _bits(a, b):
    """Bit-for-bit equality of two tensors (NaN equals the same NaN, -0.0 differs from +0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(w), b.to(a.device).contiguous().view(w))


def _tasks(n):
    return [f"t{i:02d}" for i in range(n)]


_RUNS = {}


def _run(sq, key, tmp_path_factory):
    """One fused run per configuration, its artifacts written once; shared by the tests and left unchanged."""
    if key in _RUNS:
        return _RUNS[key]
    from oracle import svd_hybrid_oracle as orc
    n, over, lacking = CONFIGS[key]
    tasks = _tasks(n)
    tv = {t: {} for t in tasks}
    for rows in ROWS:
        for t, d in zip(tasks, orc.synthetic_deltas(rows, n, 31 * n + rows, rank=min(3, n))):
            tv[t][f"p{rows:05d}"] = d.cuda()
    for name in lacking:
        del tv[tasks[3]][name]
    kw = dict(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2)
    kw.update(over)
    cfg = sq.SVDHybridConfig(**kw)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    shapes = {f"p{rows:05d}": torch.Size([rows]) for rows in ROWS}
    d = str(tmp_path_factory.mktemp(key) / "art")
    diag = {"per_parameter": {name: {"original_shape": list(s)} for name, s in shapes.items()}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    _RUNS[key] = (cfg, bases, comp, shapes, d, tasks)
    return _RUNS[key]


def _small_of(plan):
    from svdq_amd.pipeline import small_views
    host = plan.small.cpu().numpy()      # the one D2H copy
    return host, small_views(host, plan.layout, plan.P, plan.N, plan.S)


# ------------------------------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("key", list(CONFIGS))
def test_round_trip_is_byte_for_byte(sq, key, tmp_path_factory):
    cfg, bases, comp, shapes, d, tasks = _run(sq, key, tmp_path_factory)
    from svdq_amd.driver import LazyArtifacts
    origin = {}
    for load_dev in ("cpu", "cuda"):
        art = sq.load_all_artifacts(d, device=load_dev)
        ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
        assert sorted(ab) == sorted(bases) == sorted(shapes) and sorted(ac) == sorted(comp)
        plans = {}
        for name in shapes:
            bm, src = ab[name]["masked"], bases[name]["masked"]
            assert isinstance(bm, LazyArtifacts) and bm._batch is not None, (name, "declined")
            assert isinstance(ac[name], LazyArtifacts) and ac[name]._batch is not None
            batch, i = bm._batch
            assert (batch.mode, batch.table, batch.from_base, batch.unit_start, batch.plan._keep) == \
                ("plain", None, False, None, None)
            k, r, rows = int(batch.small.k[i]), int(batch.small.r[i]), int(batch.small.rows[i])
            U_high, U_low, mean = batch.plan.basis_tensors(i, k, r, rows)
            assert U_high.dtype == src["U_high"].dtype and _bits(U_high, src["U_high"]), name
            assert U_low.shape == src["U_low"].shape and _bits(U_low, src["U_low"]), name
            assert (mean is None) == (src["mean"] is None) and (mean is None or _bits(mean, src["mean"])), name
            # the dictionaries: same keys, same values, same dtypes as what was loaded
            loaded = art["bases"][name]["masked"]
            assert list(bm.keys()) == list(loaded.keys())
            for f, v in loaded.items():
                if isinstance(v, torch.Tensor):
                    assert bm[f].dtype == v.dtype and bm[f].shape == v.shape and _bits(bm[f], v.cuda()), (name, f)
                else:
                    assert type(bm[f]) is type(v) and bm[f] == v, (name, f)
            plans.setdefault(id(batch.plan), (batch.plan, []))[1].append((name, i))
        assert len(plans) == (2 if key == "missing" else 1)
        # the adopted plan's DEVICE small buffer against the originating plan's, field by field
        for plan, members in plans.values():
            host, a = _small_of(plan)
            assert not a.coef.any()
            assert int(host[plan.layout.status_off:plan.layout.status_off + 4].view(np.int32)[0]) == 0
            for name, i in members:
                ob, oi = bases[name]["masked"]._batch
                if id(ob.plan) not in origin:
                    origin[id(ob.plan)] = _small_of(ob.plan)[1]
                o = origin[id(ob.plan)]
                k, r = int(o.k[oi]), int(o.r[oi])
                n_low = r - k
                assert (int(a.k[i]), int(a.r[i]), int(a.rows[i])) == (k, r, int(o.rows[oi])), name
                assert a.energy[i:i + 1].tobytes() == o.energy[oi:oi + 1].tobytes(), name
                assert a.sigma[i, :r].tobytes() == o.sigma[oi, :r].tobytes(), name
                assert a.c_high[i, :, :k].tobytes() == o.c_high[oi, :, :k].tobytes(), name
                assert a.codes[i, :, :, :n_low].tobytes() == o.codes[oi, :, :, :n_low].tobytes(), name
                for f in ("scale", "zero_point", "residual_norm"):
                    assert getattr(a, f)[i].tobytes() == getattr(o, f)[oi].tobytes(), (name, f)
                assert plan.bits_of(i) == ob.plan.bits_of(oi)
        # the per-task artifacts are the caller's own objects
        name = "p04097"
        assert list(ac[name].keys()) == list(art["compressed"][name].keys())
        assert all(ac[name][t] is art["compressed"][name][t] for t in ac[name])


# ------------------------------------------------------------------------------------------ 2. no stray writes
@pytest.mark.parametrize("n_tasks", TASK_COUNTS)
@pytest.mark.parametrize("fp16,center", [(True, True), (True, False), (False, True), (False, False)])
def test_import_writes_the_three_ranges_and_nothing_else(sq, n_tasks, fp16, center):
    """Plan level, on a buffer pre-filled with 0xA5: after svdq_plan_import the whole allocation -- alignment gaps, slab
    tails, the buffers' tails and the slab of a parameter whose rows are 0 in the small buffer -- is 0xA5 except the
    U_high / U_low / mean ranges, which hold the sources' bytes."""
    from svdq_amd.pipeline import CompressPlan, pack_small
    rows_all = ROWS + [513]                                # the last one is skipped through rows = 0
    P, N, S = len(rows_all), n_tasks, 2
    plan = CompressPlan(rows_all, N, fp16=fp16, center=center, rtvq_stages=S, device="cuda", workspace=False)
    assert plan.workspace is None
    dt = torch.float16 if fp16 else torch.float32
    es = 2 if fp16 else 4
    g = torch.Generator().manual_seed(1000 * n_tasks + 2 * fp16 + center)
    entries, uh, ul, mn = [], [], [], []
    for p, rows in enumerate(rows_all):
        r = min(rows, N)
        k = (0, 1, r // 2, r, max(r - 1, 0))[p % 5]
        k = min(k, r)
        # byte patterns that never read 0xA5A5: small positive values
        uh.append((torch.rand(rows, k, generator=g) + 0.5).to(dt).cuda())
        ul.append((torch.rand(rows, r - k, generator=g) + 0.5).to(dt).cuda())
        mn.append((torch.rand(rows, generator=g) + 0.5).cuda())
        if p == P - 1:
            entries.append(None)
            continue
        entries.append({"rows": rows, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
                        "c_high": np.ones((N, k), np.float16), "codes": np.ones((N, S, r - k), np.uint8),
                        "scale": np.ones((N, S), np.float32), "zero_point": np.zeros((N, S), np.float32),
                        "residual_norm": np.ones((N, S), np.float32)})
    whole = torch.empty(0, dtype=torch.uint8, device="cuda").set_(plan.basis.untyped_storage())
    whole.fill_(0xA5)
    want = whole.cpu().numpy().copy()
    b0 = plan.basis.storage_offset()
    m0 = plan.mean.storage_offset() * 4 if center else None
    for p, e in enumerate(entries):
        if e is None:
            continue
        rows, k, r = e["rows"], e["k"], e["r"]
        hi = uh[p].cpu().numpy().reshape(-1).view(np.uint8)
        lo = ul[p].cpu().numpy().reshape(-1).view(np.uint8)
        o = b0 + plan.slab_off[p]
        want[o:o + hi.size] = hi
        o += (rows * k * es + 255) // 256 * 256
        want[o:o + lo.size] = lo
        if center:
            o = m0 + plan.mean_off[p] * 4
            want[o:o + rows * 4] = mn[p].cpu().numpy().view(np.uint8)
    small_host = pack_small(plan.layout, P, N, S, entries)
    plan.import_artifacts(uh, ul, mn if center else None, small_host)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(plan.small.cpu().numpy(), small_host)          # the small buffer is only read
    # what the host can see is refused: wrong dtype, a source that is not 16-byte aligned, a missing mean
    with pytest.raises(ValueError):
        plan.import_artifacts([u.double() for u in uh], ul, mn if center else None, small_host)
    q = next(p for p in range(P) if ul[p].numel() >= 8 or uh[p].numel() >= 8)
    src = uh if uh[q].numel() >= 8 else ul
    off = torch.zeros(src[q].numel() + 8, dtype=dt, device="cuda")[1:1 + src[q].numel()].view(src[q].shape)
    moved = src[:q] + [off] + src[q + 1:]
    with pytest.raises(ValueError):
        plan.import_artifacts(moved if src is uh else uh, moved if src is ul else ul, mn if center else None, small_host)
    with pytest.raises(ValueError):
        plan.import_artifacts(uh, ul, None if center else mn, small_host)
    lib = sq._native.lib()
    assert lib.svdq_plan_import(plan._h, None, None, None, None, None, None, None) == sq._native.SVDQ_EINVAL


# ------------------------------------------------------------------------------------------ 3. merges
def _weights(tasks, uniform):
    if uniform:
        return {t: 1.0 / len(tasks) for t in tasks}
    return {t: 0.15 + 0.07 * ((5 * i) % 7) for i, t in enumerate(tasks)}      # non-uniform, does not sum to 1


@pytest.mark.parametrize("key", list(CONFIGS))
def test_merges_over_adopted_artifacts_are_the_resident_merges(sq, key, tmp_path_factory):
    cfg, bases, comp, shapes, d, tasks = _run(sq, key, tmp_path_factory)
    from svdq_amd import merge as mg
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    for uniform in (True, False):
        w = _weights(tasks, uniform)
        want = sq.merge_all_parameters(comp, bases, {}, w, shapes, cfg, device="cuda", verbose=False)
        assert len(mg._merge_batched(sorted(ac), ac, ab, {}, ([(w, None)], None), shapes, cfg, "cuda")) == len(shapes)
        got = sq.merge_all_parameters(ac, ab, {}, w, shapes, cfg, device="cuda", verbose=False)
        assert sorted(got) == sorted(want) == sorted(shapes)
        for name in shapes:
            assert got[name].shape == shapes[name] and _bits(got[name], want[name]), (name, uniform)
    if len(tasks) >= 2:
        assign = {t: i % 2 for i, t in enumerate(tasks)}
        w = _weights(tasks, False)
        members = {c: [t for t in tasks if assign[t] == c] for c in (0, 1)}
        assert mg._merge_with_clustering_batched(ac, ab, {}, w, members, shapes, cfg, "cuda") is not None
        want = sq.merge_with_clustering(comp, bases, {}, w, assign, shapes, cfg, device="cuda")
        got = sq.merge_with_clustering(ac, ab, {}, w, assign, shapes, cfg, device="cuda")
        for name in shapes:
            assert _bits(got[name], want[name]), name


def test_masked_merge_over_adopted_artifacts(sq, tmp_path):
    """Signal and noise regions, masks of density 0.6 handed to the merge (they are not stored): the adopted plans take
    the compacted-rows route and give the fused run's bits."""
    from oracle import svd_hybrid_oracle as orc
    from svdq_amd import merge as mg
    tasks = _tasks(8)
    sizes = {"m04097": 4097, "m70001": 70001}
    g = torch.Generator().manual_seed(6)
    tv = {t: {} for t in tasks}
    masks = {}
    for name, rows in sizes.items():
        for t, x in zip(tasks, orc.synthetic_deltas(rows, 8, 77 + rows)):
            tv[t][name] = x.cuda()
        masks[name] = (torch.rand(rows, generator=g) < 0.6).cuda()
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2,
                             svd_include_noise=True, svd_noise_shrink=0.5, svd_min_mask_size=10)
    bases, comp = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    shapes = {n: torch.Size([r]) for n, r in sizes.items()}
    d = str(tmp_path / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()}}, cfg, d)
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    for name in sizes:
        assert ab[name]["masked"]._batch is not None and ab[name]["noise"]._batch is not None
        for region in ("masked", "noise"):
            src = bases[name][region]
            batch, i = ab[name][region]._batch
            U_high, U_low, mean = batch.plan.basis_tensors(i, int(src["k"]), int(src["k"]) + src["U_low"].shape[1], src["D"])
            assert _bits(U_high, src["U_high"]) and _bits(U_low, src["U_low"]) and _bits(mean, src["mean"])
    w = _weights(tasks, False)
    assert len(mg._merge_batched(sorted(ac), ac, ab, masks, ([(w, None)], None), shapes, cfg, "cuda")) == 2
    want = sq.merge_all_parameters(comp, bases, masks, w, shapes, cfg, device="cuda", verbose=False)
    got = sq.merge_all_parameters(ac, ab, masks, w, shapes, cfg, device="cuda", verbose=False)
    for name in sizes:
        assert _bits(got[name], want[name]), name
        assert not _bits(got[name], torch.zeros_like(got[name]))


# ------------------------------------------------------------------------------------------ 4. the route is taken
def test_reconstruct_from_artifacts_takes_the_batched_route(sq, tmp_path):
    """Counters on the library's own entry points around reconstruct_from_artifacts: one svdq_plan_import and one
    svdq_merge per plan, no per-parameter svdq_reconstruct, no per-task svdq_rtvq_dequantize."""
    from oracle import svd_hybrid_oracle as orc
    tasks = ["A", "B", "C", "D", "E", "F"]
    shapes = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (32, 64)}
    tv = {t: {} for t in tasks}
    for pi, (n, shp) in enumerate(sorted(shapes.items())):
        for t, x in zip(tasks, orc.synthetic_deltas(int(np.prod(shp)), len(tasks), 500 + pi)):
            tv[t][n] = x.view(shp).cuda()
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    weights = {t: 0.1 + 0.05 * i for i, t in enumerate(tasks)}
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()}, "task_weights": weights}
    d = str(tmp_path / "art")
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    base = {n: torch.randn(s).cuda() for n, s in shapes.items()}
    lib = sq._native.lib()
    names = ("svdq_reconstruct", "svdq_rtvq_dequantize", "svdq_plan_import", "svdq_merge")
    real = {n: getattr(lib, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def spy(n):
        def call(*a):
            calls[n] += 1
            return real[n](*a)
        return call
    for n in names:
        setattr(lib, n, spy(n))
    try:
        res = sq.reconstruct_from_artifacts(d, base, None, device="cuda")
    finally:
        for n in names:
            setattr(lib, n, real[n])
    assert calls == {"svdq_reconstruct": 0, "svdq_rtvq_dequantize": 0, "svdq_plan_import": 1, "svdq_merge": 1}, calls
    merged = sq.merge_all_parameters(comp, bases, {}, weights, {n: torch.Size(s) for n, s in shapes.items()}, cfg,
                                     device="cuda", verbose=False)
    want = sq.apply_merged_deltas(base, merged, device="cuda", verbose=False)
    assert sorted(res["merged_state_dict"]) == sorted(want)
    for n in shapes:
        assert _bits(res["merged_state_dict"][n], want[n]), n


# ------------------------------------------------------------------------------------------ 5. declined and edited
def _synthetic_entry(n_tasks, D, k, seed):
    """Artifacts built by hand, the basis from torch.linalg.qr: (basis file, coefficient file) of one parameter."""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(D, n_tasks, generator=g))
    n_low = n_tasks - k
    basis = {"masked": {"U_high": Q[:, :k].contiguous().half(), "U_low": Q[:, k:].contiguous().half(),
                        "singular_values": torch.linspace(2.0, 0.1, n_tasks), "k": k,
                        "mean": torch.randn(D, 1, generator=g) * 0.01, "energy_retained": 0.9, "D": D, "N": n_tasks}}
    coeffs = {}
    for t in range(n_tasks):
        pays = [{"stage": s, "quantized": torch.randint(0, 16, (n_low,), generator=g, dtype=torch.uint8),
                 "scale": torch.tensor(40.0 * (s + 1)), "zero_point": torch.tensor(7.5), "residual_norm": 0.1}
                for s in range(2)]
        coeffs[f"s{t:02d}"] = {"masked": {"c_high_fp16": torch.randn(k, generator=g).half(),
                                          "c_low_quant": {"payloads": pays, "num_bits": 4, "num_stages": 2,
                                                          "original_shape": torch.Size([n_low]),
                                                          "original_dtype": "torch.float32"}}}
    return basis, coeffs


def test_declined_and_edited_entries_fall_back_quietly(sq, tmp_path_factory):
    """A parameter adoption declines is handed back as it came and served by the per-parameter route, beside adopted
    ones.  Two of them here: a 33-task parameter (hand-built), and one whose U_low lost a column after loading.  The
    per-parameter route itself refuses the latter (reconstruct_from_coefficients: "Shape mismatch", as the reference's
    matrix product would), so what is compared for it is that refusal: the same error from the adopted dictionaries as
    from the loaded ones."""
    from svdq_amd import merge as mg
    from svdq_amd.driver import LazyArtifacts
    cfg, bases, comp, shapes, d, tasks = _run(sq, "n8-fp16-center", tmp_path_factory)
    art = sq.load_all_artifacts(d, device="cpu")
    lb, lc = art["bases"], art["compressed"]
    cut = "p00256"
    lb[cut]["masked"]["U_low"] = lb[cut]["masked"]["U_low"][:, :-1].contiguous()
    big_b, big_c = _synthetic_entry(33, 500, 2, 5)
    lb["big"], lc["big"] = big_b, big_c
    shapes = dict(shapes, big=torch.Size([500]))
    ab, ac = sq.adopt_artifacts(lb, lc, cfg, device="cuda")
    for name in shapes:
        adopted = isinstance(ac[name], LazyArtifacts)
        assert adopted == (name not in (cut, "big")), name
        if not adopted:
            assert ab[name] is lb[name] and ac[name] is lc[name]                  # as given
            assert mg._batched_entry(name, ac, ab) is None
        else:
            assert mg._batched_entry(name, ac, ab) is not None
    w = dict(_weights(tasks, False), **{f"s{t:02d}": 0.01 * (t + 1) for t in range(33)})
    q = sq.RTVQQuantizer(num_bits=cfg.svd_low_bits, num_stages=cfg.svd_rtvq_stages)
    for dicts in ((ac, ab), (lc, lb)):
        with pytest.raises(ValueError, match="Shape mismatch"):
            sq.merge_parameter(cut, dicts[0][cut], dicts[1][cut], w, q, shapes[cut], device="cuda")
    rest = [n for n in shapes if n != cut]
    sub = lambda m: {n: m[n] for n in rest}                                     # noqa: E731
    got = sq.merge_all_parameters(sub(ac), sub(ab), {}, w, shapes, cfg, device="cuda", verbose=False)
    for name in rest:      # the per-parameter route, parameter by parameter, from the dictionaries as loaded
        want = sq.merge_parameter(name, lc[name], lb[name], w, q, shapes[name], device="cuda")
        assert _bits(got[name], want), name
    assert float(got["big"].abs().max()) > 0
    # looking at an adopted entry (which materialises it) does not cost it the batched route
    assert list(ac["p00013"]) == tasks and ac["p00013"]["t01"] is lc["p00013"]["t01"]
    assert mg._batched_entry("p00013", ac, ab) is not None
    # an assignment into an adopted entry (a mutator): that parameter goes per parameter again, the result stays
    name = "p04097"
    ac[name]["t00"] = ac[name]["t00"]
    assert mg._batched_entry(name, ac, ab) is None and mg._batched_entry("p08193", ac, ab) is not None
    again = sq.merge_all_parameters(sub(ac), sub(ab), {}, w, shapes, cfg, device="cuda", verbose=False)
    for n in rest:
        assert _bits(again[n], got[n]), n
