"""
The task Gram as a by-product of the compressor's first pass (svdq_plan_set_task_gram / svdq_plan_task_gram).

  * a plan with the by-product writes the same artifacts, byte for byte, as the plan without it;
  * the Gram it returns is sum_p X_p X_p^T of the tensors pass 1 read, to the bound svdq_task_gram is held to
    (rtol 2e-6, atol 2e-6 max|G|), exactly symmetric, for mean-free and mean-dominated inputs alike;
  * center = 0, N <= 16: the very sums of svdq_task_gram; half inputs: the bits of their fp32 upcasts;
  * the staged entry points, the order relative to pass 2, a second run on the same plan, the refusals.
"""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu
N_LIST = [1, 2, 3, 5, 8, 13, 16, 17, 20, 24, 32]
D_LIST = [1, 3, 255, 256, 257, 4096 + 5]
BIG = 4 * 1024 * 1024 + 3          # several work units
SETTINGS = dict(energy_threshold=0.9, max_rank=None, low_bits=4, rtvq_stages=2)


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _dev():
    return torch.device("cuda", 0)


def _deltas(D, N, seed, dtype=torch.float32, common=0.0, mean_free=False):
    """N task tensors of D elements: a rank-3 signal plus noise (spread ~1), plus ``common`` times a component shared by
    all tasks; ``mean_free``: the mean over tasks is taken out of every row."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = _dev()
    r = min(3, N)
    A = torch.randn(D, r, generator=g, device=dev) @ torch.randn(r, N, generator=g, device=dev)
    A = A + 0.05 * torch.randn(D, N, generator=g, device=dev)
    if mean_free:
        A = A - A.mean(dim=1, keepdim=True)
    if common:
        A = A + common * torch.randn(D, 1, generator=g, device=dev)
    # .clone(): a storage of its own (a one-row column is a contiguous view into A at an unaligned offset)
    return [A[:, t].to(dtype).clone() for t in range(N)]


def _gram_ref(params, rows=None):
    """sum_p X_p X_p^T in fp64 (X_p = [N, rows_p]) from the tensors themselves."""
    N = len(params[0])
    G = torch.zeros((N, N), dtype=torch.float64, device=_dev())
    for p, vs in enumerate(params):
        n = vs[0].numel() if rows is None else rows[p]
        X = torch.stack([v[:n].double() for v in vs])
        G += X @ X.T
    return G.cpu().numpy()


def _check_gram(G, Gref):
    G = G.cpu().numpy() if isinstance(G, torch.Tensor) else G
    # the bound svdq_task_gram is held to (test_hip_merge.py, test_hip_fullsize.py)
    np.testing.assert_allclose(G, Gref, rtol=2e-6, atol=2e-6 * np.abs(Gref).max())
    np.testing.assert_array_equal(G, G.T)


def _plan(sq, params, center, fp16, task_gram, dtype=torch.float32, **kw):
    N = len(params[0])
    return sq.pipeline.CompressPlan([vs[0].numel() for vs in params], N, center=center, fp16=fp16, device=_dev(),
                                    input_dtype=dtype, task_gram=task_gram, **{**SETTINGS, **kw})


def _run(sq, params, center, fp16, task_gram, base=None, dtype=torch.float32, rows_dev=None):
    """One compress step; returns (plan, Gram or None).  ``base``: one tensor per parameter, params are fine-tuned."""
    plan = _plan(sq, params, center, fp16, task_gram, dtype)
    table = plan.pointer_table(params)
    if base is not None:
        btab = torch.tensor([b.data_ptr() for b in base], dtype=torch.int64).to(_dev())
        plan.run_from_base(table, btab, rows_dev)
    else:
        plan.run(table, rows_dev)
    G = plan.compress_task_gram() if task_gram else None
    torch.cuda.synchronize()
    return plan, G


def _regions(plan):
    """The bytes a run writes: the whole small buffer, and per parameter U_high, U_low and the mean (the packed buffers
    also hold never-written alignment gaps)."""
    L, P = plan.layout, plan.P
    sm = plan.small.cpu()
    k = sm[L.k_off:L.k_off + 4 * P].view(torch.int32).tolist()
    r = sm[L.r_off:L.r_off + 4 * P].view(torch.int32).tolist()
    rows = sm[L.rows_off:L.rows_off + 8 * P].view(torch.int64).tolist()
    es = 2 if plan.fp16 else 4
    out = [plan.small]
    for p in range(P):
        s, hi = plan.slab_off[p], rows[p] * k[p] * es
        out.append(plan.basis[s:s + hi])
        lo = s + (hi + 255) // 256 * 256
        out.append(plan.basis[lo:lo + rows[p] * (r[p] - k[p]) * es])
        if plan.center:
            out.append(plan.mean[plan.mean_off[p]:plan.mean_off[p] + rows[p]].view(torch.uint8))
    return out


def _same_bytes(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.numel() == y.numel() and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"region {i} differs"


def _same_layout(a, b):
    assert a.slab_off == b.slab_off and a.mean_off == b.mean_off
    for f in ("basis_bytes", "mean_floats", "small_bytes", "n_units", "n_slots"):
        assert getattr(a.sizes, f) == getattr(b.sizes, f), f
    assert a.sizes.workspace_bytes >= b.sizes.workspace_bytes
    assert bytes(a.layout) == bytes(b.layout)


# ------------------------------------------------------------------------------------------------ checks 1 + 2
@pytest.mark.parametrize("from_base", [False, True], ids=["deltas", "from_base"])
@pytest.mark.parametrize("N", N_LIST)
def test_artifacts_unchanged_and_gram_right(sq, N, from_base):
    for center, fp16 in [(True, True), (True, False), (False, True), (False, False)]:
        Ds = D_LIST + ([BIG] if (center and fp16) else [])
        deltas = [_deltas(D, N, 1000 * N + i, common=(3.0 if i % 2 else 0.0)) for i, D in enumerate(Ds)]
        base = None
        params = deltas
        if from_base:
            base = [_deltas(D, 1, 77 + i)[0] * 3.0 for i, D in enumerate(Ds)]
            params = [[b + d for d in ds] for b, ds in zip(base, deltas)]
            deltas = [[f - b for f in fs] for b, fs in zip(base, params)]     # what the kernels form
        a, G = _run(sq, params, center, fp16, True, base=base)
        b, _ = _run(sq, params, center, fp16, False, base=base)
        _same_layout(a, b)
        _same_bytes(_regions(a), _regions(b))
        _check_gram(G, _gram_ref(deltas))
        a.close()
        b.close()


CASES = {
    "mean_free": dict(mean_free=True),
    "no_common": dict(),
    "common_x10": dict(common=10.0),
    "common_x1000": dict(common=1000.0),          # s 1 1^T is nearly all of G
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("N", [3, 8, 16, 20, 32])
def test_gram_from_mean_free_to_mean_dominated(sq, N, case):
    Ds = [2, 4096 + 5, 300 * 1024 + 17]          # the first parameter has fewer rows than most N
    params = [_deltas(D, N, 31 * N + i, **CASES[case]) for i, D in enumerate(Ds)]
    plan, G = _run(sq, params, True, True, True)
    _check_gram(G, _gram_ref(params))
    plan.close()


@pytest.mark.parametrize("N", [1, 2, 5, 12, 20, 28])
def test_fewer_rows_than_tasks_and_short_rows_dev(sq, N):
    Ds = [1, 3, 4096 + 5, 70001]
    params = [_deltas(D, N, 7 * N + i, common=2.0) for i, D in enumerate(Ds)]
    rows = [1, 2, 1000, 65536 + 3]               # rows_dev shorter than the plan's rows
    rows_dev = torch.tensor(rows, dtype=torch.int64, device=_dev())
    for center in (True, False):
        a, G = _run(sq, params, center, True, True, rows_dev=rows_dev)
        b, _ = _run(sq, params, center, True, False, rows_dev=rows_dev)
        _same_bytes(_regions(a), _regions(b))
        _check_gram(G, _gram_ref(params, rows))
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ check 3
@pytest.mark.parametrize("N", [n for n in N_LIST if n <= 16])
def test_uncentred_plan_bit_equal_to_task_gram(sq, N):
    Ds = D_LIST + [BIG // 4]
    params = [_deltas(D, N, 50 * N + i, common=1.0) for i, D in enumerate(Ds)]
    plan, G = _run(sq, params, False, True, True)
    ref = sq.pipeline.CompressPlan(Ds, N, center=False, device=_dev(), gram_only=True)
    Gt = ref.task_gram(ref.pointer_table(params))
    assert torch.equal(G, Gt)       # same kernel, same partials, same reduction order
    plan.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ check 4
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [1, 5, 8, 16, 20, 32])
@pytest.mark.parametrize("from_base", [False, True], ids=["deltas", "from_base"])
def test_half_inputs_bit_equal_to_upcast(sq, N, dtype, from_base):
    Ds = D_LIST + [70001]
    half = [_deltas(D, N, 90 * N + i, dtype=dtype, common=1.5) for i, D in enumerate(Ds)]
    base = [_deltas(D, 1, 55 + i, dtype=dtype)[0] for i, D in enumerate(Ds)] if from_base else None
    for center in (True, False):
        a, Ga = _run(sq, half, center, True, True, base=base, dtype=dtype)
        b, Gb = _run(sq, [[v.float() for v in vs] for vs in half], center, True, True,
                     base=[x.float() for x in base] if from_base else None)
        assert torch.equal(Ga, Gb)
        _same_bytes(_regions(a), _regions(b))
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ check 5
def _gap_params(N_extra_seed):
    """N = 20: the reference-generated spectra that make the eigen stage flag a parameter for the exact-product
    relaunch, between ordinary parameters that it does not flag."""
    ga, gb = load_golden("spectrum_gap_n20a.npz"), load_golden("spectrum_gap_n20b.npz")
    dev = _dev()
    pa = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in ga["deltas"]]
    pb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in gb["deltas"]]
    return [_deltas(4096 + 5, 20, N_extra_seed, common=1.0), pa, _deltas(70001, 20, N_extra_seed + 1), pb,
            _deltas(257, 20, N_extra_seed + 2, common=5.0)]


@pytest.mark.parametrize("N", [3, 8, 16, 20, 32])
def test_staged_entry_points_and_order(sq, N):
    Ds = [257, 4096 + 5, 70001, 3, 300 * 1024 + 17]
    params = _gap_params(5) if N == 20 else [_deltas(D, N, 11 * N + i, common=2.0) for i, D in enumerate(Ds)]
    whole, G = _run(sq, params, True, True, True)
    Gref = _gram_ref(params)
    _check_gram(G, Gref)
    plan = _plan(sq, params, True, True, True)
    table = plan.pointer_table(params)
    st = torch.cuda.current_stream()
    P, h = plan.P, plan.P // 2
    for p0, n in ((0, h), (h, P - h)):
        plan.gram_range(table, p0, n, st)
        plan.eig_range(table, p0, n, st)
    before = plan.compress_task_gram()
    plan.basis_project(table)
    plan.coeff_quantize()
    after = plan.compress_task_gram()
    torch.cuda.synchronize()
    assert torch.equal(before, G) and torch.equal(after, G)
    _same_bytes(_regions(plan), _regions(whole))
    # a second run on the same plan, other inputs: their Gram, nothing left of the first
    if N == 20:       # the two gap spectra change places, the ordinary parameters are new
        fresh_params = _gap_params(9)
        other = [fresh_params[0], params[3], fresh_params[2], params[1], fresh_params[4]]
    else:
        other = [_deltas(D, N, 13 * N + i, common=0.5 * i) for i, D in enumerate(Ds)]
    plan.run(plan.pointer_table(other))
    G2 = plan.compress_task_gram()
    fresh, G2ref = _run(sq, other, True, True, True)
    torch.cuda.synchronize()
    assert torch.equal(G2, G2ref)
    _check_gram(G2, _gram_ref(other))
    _same_bytes(_regions(plan), _regions(fresh))
    for x in (whole, plan, fresh):
        x.close()


# ------------------------------------------------------------------------------------------------ check 6
def test_refusals(sq):
    nat, dev = sq._native, _dev()
    lib = nat.lib()
    params = [_deltas(4096, 4, 1)]
    on = _plan(sq, params, True, True, True)
    off = _plan(sq, params, True, True, False)
    junk = torch.zeros(4096, dtype=torch.int64, device=dev)
    p = c_void_p(junk.data_ptr())
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    h = on._h
    guard = on.small.clone()
    calls = {
        "svdq_compress_gather": lambda: lib.svdq_compress_gather(h, p, p, p, p, p, p, p, st),
        "svdq_compress_gather_from_base": lambda: lib.svdq_compress_gather_from_base(h, p, p, p, p, p, p, p, p, st),
        "svdq_compress_masked": lambda: lib.svdq_compress_masked(h, p, p, p, p, p, p, p, p, st),
        "svdq_compress_masked_from_base": lambda: lib.svdq_compress_masked_from_base(h, p, p, p, p, p, p, p, p, p, st),
    }
    for name, call in calls.items():
        assert call() == nat.SVDQ_EUNSUPPORTED, name
        assert name in nat.last_error(), nat.last_error()
    out = torch.full((4, 4), -7.0, dtype=torch.float64, device=dev)
    o = c_void_p(out.data_ptr())
    w = c_void_p(off.workspace.data_ptr())
    assert lib.svdq_plan_task_gram(off._h, w, o, st) == nat.SVDQ_EINVAL
    assert "svdq_plan_set_task_gram" in nat.last_error()
    w = c_void_p(on.workspace.data_ptr())
    assert lib.svdq_plan_task_gram(None, w, o, st) == nat.SVDQ_EINVAL
    assert lib.svdq_plan_task_gram(h, None, o, st) == nat.SVDQ_EINVAL
    assert lib.svdq_plan_task_gram(h, w, None, st) == nat.SVDQ_EINVAL
    assert lib.svdq_plan_set_task_gram(None, 1) == nat.SVDQ_EINVAL
    torch.cuda.synchronize()
    # nothing was enqueued by a refused call
    assert torch.equal(out, torch.full_like(out, -7.0)) and torch.equal(on.small, guard)
    with pytest.raises(ValueError):
        off.compress_task_gram()
    on.close()
    off.close()


# ------------------------------------------------------------------------------------------------ check 7: host flow
class _Spy:
    """Counts svdq_task_gram calls on the ctypes table and records the rows of the plans made for them."""

    def __init__(self, sq, monkeypatch):
        self.calls, self.rows = 0, []
        lib = sq._native.lib()
        real = lib.svdq_task_gram
        Plan = sq.pipeline.CompressPlan
        spy = self

        def counted(*a):
            spy.calls += 1
            return real(*a)

        class Recording(Plan):
            def __init__(self, rows, *a, **kw):
                if kw.get("gram_only"):
                    spy.rows.append(list(rows))
                super().__init__(rows, *a, **kw)

        monkeypatch.setattr(lib, "svdq_task_gram", counted, raising=False)
        monkeypatch.setattr(sq.clustering, "CompressPlan", Recording)


def _cluster_config(sq, **kw):
    cfg = sq.SVDHybridConfig(svd_energy_threshold=0.9, svd_center=True, svd_fp16=True, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_weighting="cluster")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _check_cluster_flow(sq, g, tv, tasks, bases):
    from test_cluster_cpu import golden_gram, same_partition
    G, names = sq.task_gram(tv, "cuda", bases=bases)
    assert names == sorted(tasks)
    _check_gram(G, golden_gram(g)[0])
    for method in ("kmeans", "hierarchical"):
        for k in (2, 3):
            lab = sq.cluster_tasks(tv, k, method=method, device="cuda", bases=bases)
            assert same_partition([lab[t] for t in tasks], g[f"labels__{method}__k{k}"]), (method, k)
    assign = {t: int(l) for t, l in zip(tasks, g["labels__kmeans__k3"])}
    st = sq.compute_cluster_statistics(tv, assign, device="cuda", bases=bases)
    for i, cid in enumerate(g["stats__cids"]):
        for key in ("mean_distance_to_centroid", "max_distance_to_centroid", "min_distance_to_centroid"):
            assert st[int(cid)][key] == pytest.approx(float(g[f"stats__{key}"][i]), rel=5e-5, abs=1e-7)


def test_cluster_flow_unmasked_reads_nothing_again(sq, monkeypatch):
    from test_hip_merge import _cluster_inputs
    g = load_golden("cluster.npz")
    tv, tasks = _cluster_inputs(g)
    cfg = _cluster_config(sq)
    bases, _ = sq.run_basis_and_compress(tv, None, cfg, "cuda")          # the cluster config is the trigger
    plain, _ = sq.run_basis_and_compress(tv, None, _cluster_config(sq, svd_weighting="uniform"), "cuda")
    assert list(bases) == list(plain)                                    # same dictionaries, same artifacts
    for name in bases:
        (ba, i), (bb, j) = bases[name]["masked"]._batch, plain[name]["masked"]._batch
        assert ba.entries == bb.entries and i == j and ba.task_names == bb.task_names
        _same_bytes(_regions(ba.plan), _regions(bb.plan))
        assert ba.task_gram is not None and getattr(bb, "task_gram", None) is None
    spy = _Spy(sq, monkeypatch)
    _check_cluster_flow(sq, g, tv, tasks, bases)
    assert spy.calls == 0
    # without the record: today's route
    sq.task_gram(tv, "cuda", bases=plain)
    assert spy.calls == 1 and len(spy.rows[-1]) == 3


def test_cluster_flow_masked_parameters_add_one_pass(sq, monkeypatch):
    from test_hip_merge import _cluster_inputs
    g = load_golden("cluster.npz")
    tv, tasks = _cluster_inputs(g)
    gen = torch.Generator(device="cuda").manual_seed(1)
    masks = {"a.weight": torch.rand(6144, generator=gen, device=_dev()) < 0.8,      # dense: walked
             "b.weight": torch.rand(3200, generator=gen, device=_dev()) < 0.2}      # sparse: index lists
    cfg = _cluster_config(sq, svd_include_noise=True, svd_min_mask_size=10)
    bases, _ = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    modes = {x[region]._batch[0].mode for x in bases.values() for region in ("masked", "noise")
             if x.get(region) is not None}
    assert modes == {"plain", "walk", "gather"}, modes
    spy = _Spy(sq, monkeypatch)
    G, _ = sq.task_gram(tv, "cuda", bases=bases)
    assert spy.calls == 1 and sorted(spy.rows[-1]) == [3200, 6144]       # the masked parameters only, in full
    _check_cluster_flow(sq, g, tv, tasks, bases)


def test_cluster_flow_from_checkpoints(sq, monkeypatch):
    N, dev = 6, _dev()
    shapes = {"w1": (300, 64), "b1": (257,), "w2": (4101,)}
    base = {n: _deltas(int(np.prod(s)), 1, 90 + j)[0].view(s) * 2.0 for j, (n, s) in enumerate(shapes.items())}
    ft = {f"t{i}": {} for i in range(N)}
    for j, (n, s) in enumerate(shapes.items()):
        ds = _deltas(int(np.prod(s)), N, 200 + j, common=0.5)
        for i in range(N):
            # two groups of tasks, so that the partition is not a toss-up
            ft[f"t{i}"][n] = (base[n].view(-1) + ds[i] + (3.0 if i % 2 else -3.0) * ds[i % 2]).view(s)
    cfg = _cluster_config(sq)
    bases, _ = sq.run_basis_and_compress_from_checkpoints(base, ft, cfg, dev)
    spy = _Spy(sq, monkeypatch)
    names_only = {t: {} for t in ft}
    got = {k: sq.cluster_tasks(names_only, k, device=dev, bases=bases) for k in (2, 3)}
    Gb, _ = sq.task_gram(names_only, dev, bases=bases)
    assert spy.calls == 0
    tv = {t: {n: (v - base[n]) for n, v in d.items()} for t, d in ft.items()}        # ingest
    from test_cluster_cpu import same_partition
    for k in (2, 3):
        want = sq.cluster_tasks(tv, k, device=dev)
        assert same_partition([got[k][t] for t in sorted(ft)], [want[t] for t in sorted(ft)]), k
    Gt, _ = sq.task_gram(tv, dev)
    np.testing.assert_allclose(Gb, Gt, rtol=2e-6, atol=2e-6 * np.abs(Gt).max())


def _as_plan(sq, plan, small, basis, mean):
    """An operator's output buffers behind the layout of ``plan`` (for _regions)."""
    view = sq.pipeline.CompressPlan.__new__(sq.pipeline.CompressPlan)
    view.__dict__.update(plan.__dict__)
    view._h = c_void_p()
    view.small, view.basis, view.mean = small, basis, mean
    return view


@pytest.mark.parametrize("N", [3, 8, 20])
def test_torch_operator_equals_ctypes_route(sq, N):
    sq.torch_ops.load()
    for center, fp16 in [(True, True), (False, False)]:
        params = [_deltas(D, N, 17 * N + i, common=1.0) for i, D in enumerate(D_LIST + [70001])]
        flat = [v for vs in params for v in vs]
        small, basis, mean, gram = torch.ops.svdq.compress_task_gram(flat, N, 0.9, 0, center, fp16, 4, 2)
        plan, G = _run(sq, params, center, fp16, True)
        assert torch.equal(gram, G)
        got = _as_plan(sq, plan, small, basis, mean if center else None)
        _same_bytes(_regions(got), _regions(plan))
        # and the plain operator writes what the by-product operator writes
        s2, b2, m2 = torch.ops.svdq.compress(flat, N, 0.9, 0, center, fp16, 4, 2)
        _same_bytes(_regions(_as_plan(sq, plan, s2, b2, m2 if center else None)), _regions(got))
        plan.close()
