"""
CPU-only checks of the host half of artifact adoption (include/svdq.h, svdq_plan_import; driver.adopt_artifacts):
``pipeline.pack_small`` -- the bytes of a plan's small-artifact buffer from per-parameter values -- against a hand-built
layout, and the rules by which adoption declines a parameter (``driver._adoptable``) or groups parameters into plans
(``driver._adoption_groups``).  No GPU, no library call.
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


# ---------------------------------------------------------------------------------------------- pack_small
P, N, S = 3, 3, 2
K = (1, 3, 0)
R = (3, 3, 2)
ROWS = (7, 4097, 2)


def _layout():
    """Offsets chosen by hand: the fields in another order than the library's, with gaps of odd sizes between them (each
    field aligned for its element type), so nothing can pass by assuming the library's arithmetic."""
    sizes = {"status": 4, "rows": P * 8, "sigma": P * N * 4, "codes": P * N * S * N, "k": P * 4, "chigh": P * N * N * 2,
             "energy": P * 4, "zp": P * N * S * 4, "r": P * 4, "coef": P * N * N * 4, "scale": P * N * S * 4,
             "rnorm": P * N * S * 4}
    off, lay = 24, {}
    for i, (name, n) in enumerate(sizes.items()):
        off = (off + 7) // 8 * 8
        lay[name + "_off"] = off
        off += n + 8 * (i % 3) + 5
    lay["total_bytes"] = off + 40
    return SimpleNamespace(**lay), sizes


def _entries():
    g = np.random.default_rng(11)
    out = []
    for p in range(P):
        k, r = K[p], R[p]
        out.append({"rows": ROWS[p], "k": k, "r": r, "energy": 0.25 + 0.125 * p,
                    "sigma": (g.random(r) + 0.5).astype(np.float32),
                    "c_high": (g.standard_normal((N, k)) + 3.0).astype(np.float16),
                    "codes": g.integers(1, 256, size=(N, S, r - k)).astype(np.uint8),
                    "scale": (g.random((N, S)) + 1.0).astype(np.float32),
                    "zero_point": (g.random((N, S)) + 2.0).astype(np.float32),
                    "residual_norm": (g.random((N, S)) + 3.0).astype(np.float32)})
    return out


def test_pack_small_round_trips_through_the_plan_slicing(sq):
    from svdq_amd.pipeline import pack_small, small_views
    L, _ = _layout()
    entries = _entries()
    buf = pack_small(L, P, N, S, entries)
    assert buf.dtype == np.uint8 and buf.shape == (L.total_bytes,)
    v = small_views(buf, L, P, N, S)      # the slicing CompressPlan.fetch_small uses
    for p, e in enumerate(entries):
        k, r = K[p], R[p]
        assert (int(v.k[p]), int(v.r[p]), int(v.rows[p])) == (k, r, ROWS[p])
        assert v.energy[p] == np.float32(e["energy"])
        assert np.array_equal(v.sigma[p, :r], e["sigma"])
        assert np.array_equal(v.c_high[p, :, :k].view(np.uint16), e["c_high"].view(np.uint16))
        assert np.array_equal(v.codes[p, :, :, :r - k], e["codes"])
        assert np.array_equal(v.scale[p], e["scale"]) and np.array_equal(v.zero_point[p], e["zero_point"])
        assert np.array_equal(v.residual_norm[p], e["residual_norm"])
    assert not v.coef.any()                                            # no stored artifact has them
    assert int(buf[L.status_off:L.status_off + 4].view(np.int32)[0]) == 0


def test_pack_small_writes_nothing_but_the_valid_elements(sq):
    from svdq_amd.pipeline import pack_small, small_views
    L, _ = _layout()
    buf = pack_small(L, P, N, S, _entries())
    # mark the valid elements through the same views on a buffer of zeros, then compare byte for byte
    cover = np.zeros(L.total_bytes, dtype=np.uint8)
    c = small_views(cover, L, P, N, S)
    for p in range(P):
        k, r = K[p], R[p]
        c.k.view(np.uint32)[p] = c.r.view(np.uint32)[p] = c.energy.view(np.uint32)[p] = 0xFFFFFFFF
        c.rows.view(np.uint64)[p] = np.uint64(0xFFFFFFFFFFFFFFFF)
        c.sigma.view(np.uint32)[p, :r] = 0xFFFFFFFF
        c.c_high.view(np.uint16)[p, :, :k] = 0xFFFF
        c.codes[p, :, :, :r - k] = 0xFF
        for f in (c.scale, c.zero_point, c.residual_norm):
            f.view(np.uint32)[p] = 0xFFFFFFFF
    assert cover.any() and not cover.all()
    assert not buf[cover == 0].any()
    # every valid element was given a value without a zero byte pattern overall: the covered part is not all zero either
    assert buf[cover != 0].any()
    # an entry of None is a skipped parameter: rows 0, everything of it zero
    again = pack_small(L, P, N, S, [None] + _entries()[1:])
    w = small_views(again, L, P, N, S)
    assert int(w.rows[0]) == 0 and int(w.k[0]) == 0 and not w.sigma[0].any() and not w.scale[0].any()
    assert np.array_equal(w.sigma[1], small_views(buf, L, P, N, S).sigma[1])
    with pytest.raises(ValueError):
        pack_small(L, P, N, S, _entries()[:2])
    bad = _entries()
    bad[0]["k"] = 4
    with pytest.raises(ValueError):
        pack_small(L, P, N, S, bad)


# ---------------------------------------------------------------------------------------------- decline rules
def _stored(n_tasks=5, D=40, k=2, n_low=3, stages=2, bits=4, dtype=torch.float16, mean=True, seed=0):
    """One region of one parameter as the artifact files hold it: (basis dictionary, artifacts of its tasks)."""
    g = torch.Generator().manual_seed(seed)
    basis = {"U_high": torch.randn(D, k, generator=g).to(dtype), "U_low": torch.randn(D, n_low, generator=g).to(dtype),
             "singular_values": torch.rand(k + n_low, generator=g), "k": k,
             "mean": torch.randn(D, 1, generator=g) if mean else None, "energy_retained": 0.9, "D": D, "N": n_tasks}
    arts = []
    for t in range(n_tasks):
        pays = [{"stage": s, "quantized": torch.randint(0, 16, (n_low,), generator=g, dtype=torch.uint8),
                 "scale": torch.tensor(1.5 + s), "zero_point": torch.tensor(0.25), "residual_norm": 0.5}
                for s in range(stages)]
        arts.append({"c_high_fp16": torch.randn(k, generator=g).half(),
                     "c_low_quant": {"payloads": pays, "num_bits": bits, "num_stages": stages,
                                     "original_shape": torch.Size([n_low]), "original_dtype": "torch.float32"}})
    return basis, arts


def test_a_stored_region_is_adoptable(sq):
    from svdq_amd.driver import _adoptable
    for kw in ({}, {"dtype": torch.float32}, {"mean": False}, {"n_tasks": 32, "D": 64, "k": 1, "n_low": 31},
               {"n_low": 0, "k": 1}, {"k": 0, "n_low": 2}, {"stages": 1}, {"stages": 8, "bits": 8}, {"bits": 1},
               {"n_tasks": 1, "k": 1, "n_low": 0}, {"D": 3, "n_tasks": 8, "k": 1, "n_low": 2}):
        assert _adoptable(*_stored(**kw)) is None, kw
    # U_low of no columns: this package writes no payloads then
    basis, arts = _stored(n_low=0, k=2)
    for a in arts:
        a["c_low_quant"]["payloads"] = []
    assert _adoptable(basis, arts) is None


def _drop_u_low_column(b, a):
    b["U_low"] = b["U_low"][:, :-1].contiguous()


def _wrong_c_high(b, a):
    a[1]["c_high_fp16"] = torch.zeros(3).half()


def _wrong_code_row(b, a):
    a[2]["c_low_quant"]["payloads"][1]["quantized"] = torch.zeros(2, dtype=torch.uint8)


def _wrong_n_low(b, a):
    a[0]["c_low_quant"]["original_shape"] = torch.Size([4])


def _payload_short(b, a):
    a[3]["c_low_quant"]["payloads"].pop()


def _bits(v):
    def edit(b, a):
        for x in a:
            x["c_low_quant"]["num_bits"] = v
    return edit


def _dtypes_differ(b, a):
    b["U_low"] = b["U_low"].float()


def _dtype_other(b, a):
    b["U_high"], b["U_low"] = b["U_high"].bfloat16(), b["U_low"].bfloat16()


def _dtype_double(b, a):
    b["U_high"], b["U_low"] = b["U_high"].double(), b["U_low"].double()


def _k_differs(b, a):
    b["k"] = 3


RULES = [
    ("more than 32 tasks", dict(n_tasks=33, D=64), None),
    ("U_high.shape[1] != k", {}, _k_differs),
    ("k + n_low != U_high.shape[1] + U_low.shape[1] (a basis column dropped)", {}, _drop_u_low_column),
    ("k + n_low != U_high.shape[1] + U_low.shape[1] (a task's n_low)", {}, _wrong_n_low),
    ("c_high_fp16 of the wrong length", {}, _wrong_c_high),
    ("a quantized row of the wrong length", {}, _wrong_code_row),
    ("payload count != num_stages", {}, _payload_short),
    ("num_bits 0", {}, _bits(0)),
    ("num_bits 9", {}, _bits(9)),
    ("U_high / U_low of different dtypes", {}, _dtypes_differ),
    ("a dtype other than fp16 / fp32: bf16", {}, _dtype_other),
    ("a dtype other than fp16 / fp32: fp64", {}, _dtype_double),
]


@pytest.mark.parametrize("what,kw,edit", RULES, ids=[r[0] for r in RULES])
def test_adoption_declines(sq, what, kw, edit):
    """One case per rule, each on a region that is adoptable but for the one thing."""
    from svdq_amd.driver import _adoptable
    basis, arts = _stored(**kw)
    if edit is not None:
        assert _adoptable(*_stored(**kw)) is None
        edit(basis, arts)
    reason = _adoptable(basis, arts)
    assert isinstance(reason, str) and reason, what


def _files(names=("a.w", "b.w", "c.w"), tasks=("t0", "t1", "t2", "t3", "t4"), **kw):
    """(bases, compressed_all) in the layout load_all_artifacts returns: only the regions that exist are keys."""
    bases, comp = {}, {}
    for i, n in enumerate(names):
        basis, arts = _stored(n_tasks=len(tasks), seed=i, **kw)
        bases[n] = {"masked": basis}
        comp[n] = {t: {"masked": a} for t, a in zip(tasks, arts)}
    return bases, comp


def test_a_task_that_lacks_a_region_is_grouped_not_declined(sq):
    """Grouping follows build_bases: the plan of a parameter holds the tasks that have it."""
    from svdq_amd.driver import _adoption_groups
    bases, comp = _files(k=2, n_low=2)            # four basis columns: four tasks can still carry them
    del comp["b.w"]["t2"]                       # the task has no entry at all for this parameter
    comp["c.w"]["t4"] = {}                      # the task is listed but holds no region (what the writer stores then)
    bases["b.w"]["masked"]["N"] = bases["c.w"]["masked"]["N"] = 4
    groups, declined = _adoption_groups(bases, comp)
    assert declined == {}
    by_n = {key[0]: [e["name"] for e in es] for key, es in groups.items()}
    assert by_n == {5: ["a.w"], 4: ["b.w", "c.w"]}
    e = {x["name"]: x for es in groups.values() for x in es}
    assert e["b.w"]["tasks"] == ["t0", "t1", "t3", "t4"] and e["c.w"]["tasks"] == ["t0", "t1", "t2", "t3"]
    assert all(len(x["artifacts"]) == len(x["tasks"]) for x in e.values())
    # what cannot be expressed: more basis columns than tasks left to carry them
    bases, comp = _files(k=2, n_low=3)
    del comp["a.w"]["t0"]
    groups, declined = _adoption_groups(bases, comp)
    assert list(declined) == ["a.w"] and "a.w" not in [x["name"] for es in groups.values() for x in es]


def test_plans_are_keyed_by_tasks_stages_dtype_and_mean(sq):
    from svdq_amd.driver import _adoption_groups
    bases, comp = {}, {}
    variants = {"p.h": {}, "p.s": {"stages": 3}, "p.f": {"dtype": torch.float32}, "p.m": {"mean": False},
                "p.b": {"bits": 8}, "p.h2": {}}
    for n, kw in variants.items():
        b, c = _files(names=(n,), **kw)
        bases.update(b)
        comp.update(c)
    # a noise region is an entry of its own, under the artifacts' "unmasked" key
    nb, na = _stored(n_tasks=5, D=24, seed=9)
    bases["p.h"]["noise"] = nb
    for t, a in zip(comp["p.h"], na):
        comp["p.h"][t]["unmasked"] = a
    groups, declined = _adoption_groups(bases, comp)
    assert declined == {}
    got = {key: [(e["name"], e["region"], e["bits"]) for e in es] for key, es in groups.items()}
    assert got == {
        (5, 2, torch.float16, False): [("p.h", "masked", 4), ("p.h", "noise", 4), ("p.b", "masked", 8), ("p.h2", "masked", 4)],
        (5, 3, torch.float16, False): [("p.s", "masked", 4)],
        (5, 2, torch.float32, False): [("p.f", "masked", 4)],
        (5, 2, torch.float16, True): [("p.m", "masked", 4)],
    }
    # a parameter goes with all its regions or not at all; the others are untouched; nothing raises on data
    broken = copy.deepcopy(bases)
    broken["p.h"]["noise"]["U_low"] = broken["p.h"]["noise"]["U_low"][:, :-1].contiguous()
    broken["p.s"]["masked"]["D"] = None
    comp["p.f"]["t1"]["masked"]["c_low_quant"] = "not a dictionary"
    groups, declined = _adoption_groups(broken, comp)
    assert sorted(declined) == ["p.f", "p.h", "p.s"] and declined["p.h"].startswith("[noise]")
    assert sorted(e["name"] for es in groups.values() for e in es) == ["p.b", "p.h2", "p.m"]


def test_adoption_is_exported(sq):
    assert callable(sq.adopt_artifacts) and callable(sq.pack_small)
    assert hasattr(sq.CompressPlan, "import_artifacts")
    assert "svdq_plan_import" in sq._native.SIGNATURES


def test_bulk_and_tensorwise_gathering_agree(sq):
    """adopt_artifacts takes a plan's small tensors to the host with one concatenation per field; the tensor-by-tensor
    path it falls back to for unusual shapes gives the same pack_small entries, value for value and dtype for dtype."""
    from svdq_amd.driver import _adoption_groups, _gather_bulk, _gather_each, _gather_small
    bases, comp = {}, {}
    tasks = [f"t{i}" for i in range(5)]
    for i, (k, n_low) in enumerate([(2, 3), (0, 4), (3, 0), (1, 1), (5, 0), (2, 2)]):
        b, arts = _stored(n_tasks=5, k=k, n_low=n_low, seed=20 + i)
        if i == 4:
            for a in arts:      # no low columns: this package stores no payloads then
                a["c_low_quant"]["payloads"] = []
        bases[f"q{i}"] = {"masked": b}
        comp[f"q{i}"] = {t: {"masked": a} for t, a in zip(tasks, arts)}
    groups, declined = _adoption_groups(bases, comp)
    assert declined == {} and len(groups) == 1
    (entries,) = groups.values()

    def same(x, y):
        assert len(x) == len(y) == len(entries)
        for ex, ey in zip(x, y):
            assert ex.keys() == ey.keys()
            for f in ex:
                ax, ay = np.asarray(ex[f]), np.asarray(ey[f])
                assert ax.dtype == ay.dtype and ax.shape == ay.shape and ax.tobytes() == ay.tobytes(), f
    each = _gather_each(entries, 5, 2)
    same(_gather_bulk(entries, 5, 2), each)
    assert each[0]["codes"].shape == (5, 2, 3) and each[0]["codes"].any() and each[2]["c_high"].shape == (5, 3)
    # scales of another shape in one task: the bulk path refuses, the front door still answers, with the same values
    entries[1]["artifacts"][2]["c_low_quant"]["payloads"][0]["scale"] = torch.tensor([2.5])
    with pytest.raises(Exception):
        _gather_bulk(entries, 5, 2)
    got = _gather_small(entries, 5, 2)
    same(got, _gather_each(entries, 5, 2))
    assert got[1]["scale"][2, 0] == np.float32(2.5)
