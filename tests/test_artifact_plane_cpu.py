"""
CPU checks of tests/artifact_plane.py: that the built plans cover the (k, r) plane where the kernels' staging geometry
changes, that the derived per-element bound holds for legitimate fp32 evaluations of the rows (three summation orders),
and that it is sharp enough to matter -- every mutation a consumer kernel could plausibly commit exceeds it on a spiked
row of every parameter it can touch.  No GPU, no library call.
"""
import numpy as np
import pytest

import artifact_plane as ap
import ties_model as tm

# (N, fp16, center, stages): every plan the GPU tests build
CASES = [(n, fp16, center, ap.STAGES) for n in ap.TASKS for fp16 in (True, False) for center in (True, False)] + \
        [(8, fp16, True, s) for fp16 in (True, False) for s in (1, 4)]
SCALE = 0.3      # not a power of two: the product rounds

_CONTENTS = {}


def _contents(case):
    if case not in _CONTENTS:
        n, fp16, center, stages = case
        _CONTENTS[case] = ap.Contents(n, fp16=fp16, center=center, stages=stages)
    return _CONTENTS[case]


def _ids(c):
    return f"n{c[0]}-{'fp16' if c[1] else 'fp32'}-{'center' if c[2] else 'nocenter'}-s{c[3]}"


# ------------------------------------------------------------------------------------------------ coverage
def test_the_plane_is_what_the_definition_says():
    assert ap.plane(1) == [(0, 1), (1, 1)]
    assert ap.plane(3) == [(0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    assert len(ap.plane(8)) == 44
    p20 = ap.plane(20)
    assert sorted({r for _, r in p20}) == [1, 10, 19, 20]
    assert [k for k, r in p20 if r == 20] == [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 19, 20]
    assert [k for k, r in p20 if r == 10] == [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]
    for n in ap.TASKS:
        pl = ap.plane(n)
        assert len(pl) == len(set(pl)) and all(0 <= k <= r <= n and r >= 1 for k, r in pl)


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("n", ap.TASKS)
def test_the_built_plans_cover_the_plane(n, fp16):
    c = _contents((n, fp16, True, ap.STAGES))
    live = [e for _, e in c.live()]
    assert sum(e is None for e in c.entries) == 1 and c.rows.count(0) == 1      # the parameter without rows
    assert all(e.U.element_size() == (2 if fp16 else 4) for e in live)
    assert all(0 <= e.k <= e.r <= min(n, e.rows) and e.r >= 1 for e in live)
    assert {e.rows for e in live} == set(ap.ROW_EDGES) | {4097, 8193}
    # every pair of the plane is there, unclamped, at some row count (r <= 32 <= max(ROW_EDGES) always) -- and so is
    # every n_low = r - k the plane has; the clamp still makes the small-row parameters
    built = {(e.k, e.r) for e in live}
    assert max(ap.ROW_EDGES) >= n and set(ap.plane(n)) <= built, sorted(set(ap.plane(n)) - built)
    assert {r - k for k, r in ap.plane(n)} <= {e.r - e.k for e in live if e.rows >= 2 or n == 1}
    assert n == 1 or any(e.r == e.rows < n for e in live)
    # every k mod 8 residue the plane can give
    assert {k % 8 for k, _ in ap.plane(n)} == {e.k % 8 for e in live}
    # k = 0, k = r and r < N, each with at least two rows
    many = [e for e in live if e.rows >= 2]
    assert any(e.k == 0 for e in many) and any(e.k == e.r for e in many)
    assert n == 1 or any(e.r < n and e.rows > e.r for e in many)
    assert n == 1 or any(0 < e.k < e.r for e in many)
    # odd k and even k, each at a 256 / 257-row edge and at a 128 / 129-row edge
    for edge in ((256, 257), (128, 129)):
        at = {e.k % 2 for e in live if e.rows in edge}
        assert at == {0, 1}, (n, edge, at)
    # the long parameters: both ends, the middle and k = 1 over several units
    long = [(e.rows, e.k, e.r) for e in live if e.rows > 4096]
    assert long == ap.long_pairs(n)
    # the two packagings hold the same values
    names, tasks, bases, comp = c.dictionaries()
    assert len(names) == len(live) and len(tasks) == n
    for name, e in zip(names, live):
        b, sm = bases[name]["masked"], e.small()
        assert b["U_high"].shape == (e.rows, e.k) and b["U_low"].shape == (e.rows, e.r - e.k) and b["k"] == e.k
        for t, task in enumerate(tasks):
            a = comp[name][task]["masked"]
            assert np.array_equal(a["c_high_fp16"].numpy().view(np.uint16), sm["c_high"][t].view(np.uint16))
            for s, pay in enumerate(a["c_low_quant"]["payloads"]):
                assert np.array_equal(pay["quantized"].numpy(), sm["codes"][t, s])
                assert float(pay["scale"]) == sm["scale"][t, s] and float(pay["zero_point"]) == sm["zero_point"][t, s]


def test_adoption_takes_every_parameter_of_the_dictionary_packaging():
    """driver._adoption_groups declines nothing and puts a store into one plan."""
    from svdq_amd.driver import _adoption_groups
    for n, fp16 in ((3, True), (17, False)):
        names, tasks, bases, comp = ap.Contents(n, fp16=fp16, center=True, zero=False).dictionaries()
        groups, declined = _adoption_groups(bases, comp)
        assert declined == {} and len(groups) == 1
        (entries,) = groups.values()
        assert [e["name"] for e in entries] == names


# ------------------------------------------------------------------------------------------------ the bound holds
def _chain(u, c, order):
    """sum_j u[:, j] c[:, j] in fp32 -- products and sums rounded one by one -- over the columns in ``order``:
    u [rows, m], c [S, m] -> [rows, S]."""
    rows, m = u.shape
    if m == 0:
        return np.zeros((rows, c.shape[0]), dtype=np.float32)
    prods = [(u[:, j:j + 1] * c[None, :, j]).astype(np.float32) for j in range(m)]
    if order == "pairwise":
        while len(prods) > 1:
            nxt = [(prods[i] + prods[i + 1]).astype(np.float32) for i in range(0, len(prods) - 1, 2)]
            if len(prods) % 2:
                nxt.append(prods[-1])
            prods = nxt
        return prods[0]
    acc = np.zeros_like(prods[0])
    for j in (range(m) if order == "forward" else reversed(range(m))):
        acc = (acc + prods[j]).astype(np.float32)
    return acc


def _fp32_rows(e, C, order, scale):
    """row_value in fp32 for the coefficient vectors C [S, r]: [rows, S]."""
    u = e.U.float().numpy()
    v = (_chain(u[:, :e.k], C[:, :e.k], order) + _chain(u[:, e.k:], C[:, e.k:], order)).astype(np.float32)
    if e.mean is not None:
        v = (v + e.mean.numpy()[:, None]).astype(np.float32)
    return (v * np.float32(scale)).astype(np.float32)


def _sets(n, seed):
    """(weights [S, N] renormalised per set with one absent task, order, softmax share) for the largest S <= min(N, 8)."""
    g = np.random.default_rng(seed)
    S = max(s for s in (1, 2, 4, 8) if s <= n)
    w = np.full((S, n), -1.0, dtype=np.float32)
    for t in range(n):
        w[t % S, t] = 0.5 + g.random()
    w[0, :] = np.where(w[0] < 0, 0.25 + g.random(n), w[0])      # set 0 holds every task ...
    if n > 1:
        w[0, n - 1] = -1.0                                       # ... but one
    for s in range(S):
        live = w[s] >= 0
        w[s, live] = (w[s, live] / w[s, live].sum(dtype=np.float32)).astype(np.float32)
    order = g.permutation(n).astype(np.int32)
    z = g.standard_normal(S)
    share = (np.exp(z) / np.exp(z).sum()).astype(np.float32)
    return w, order, share


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_the_bound_holds_for_fp32_evaluations_in_three_orders(case):
    c = _contents(case)
    g = np.random.default_rng(case[0])
    w, order, share = _sets(c.n, 5)
    checked = 0
    for p, e in c.live():
        base = g.standard_normal(e.rows).astype(np.float32)
        C = ap.coefs(e)
        want, bound = ap.task_rows(e, SCALE, base, C=C)
        assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound > 0).all(), (p, e.rows, e.k, e.r)
        mw, mb = ap.merged_rows(e, w, order, share, SCALE, base)
        assert np.isfinite(mw).all()
        cb = ap.cbar(e, w, order, C=C)
        for how in ("forward", "backward", "pairwise"):
            got = (base[:, None] + _fp32_rows(e, C, how, SCALE)).astype(np.float32)
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (p, e.rows, e.k, e.r, how, float((err / bound).max()))
            v = _fp32_rows(e, cb, how, SCALE)
            res = np.zeros(e.rows, dtype=np.float32)
            for s in range(share.size):
                res = (res + (v[:, s] * share[s]).astype(np.float32)).astype(np.float32)
            got = (base + res).astype(np.float32)
            err = np.abs(got.astype(np.float64) - mw)
            assert (err <= mb).all(), (p, e.rows, e.k, e.r, how, "merged", float((err / mb).max()))
        checked += 1
    assert checked == len(c.params) - 1      # no parameter left out but the one without rows


def test_the_coefficient_model_is_the_dequantizer_in_torch_fp32():
    """coef against the dequantizer's lines restated with torch fp32 tensor operations on the payloads of the
    dictionary packaging (zeros, + (q.float() - zero_point) / scale per stage): the same bits.  The GPU test holds the
    device's RTVQQuantizer.dequantize to the same."""
    import torch
    c = _contents((8, True, True, 4))
    for p, e in c.live():
        for t in (0, e.n - 1):
            q = e.task_dict(t)["c_low_quant"]
            want = torch.zeros(e.r - e.k, dtype=torch.float32)
            for pay in q["payloads"]:
                want = want + (pay["quantized"].float() - pay["zero_point"]) / pay["scale"]
            got = ap.coef(e, t)
            assert np.array_equal(got[e.k:].view(np.uint32), want.numpy().view(np.uint32)), (p, t)
            assert np.array_equal(got[:e.k], e.task_dict(t)["c_high_fp16"].float().numpy())


# ------------------------------------------------------------------------------------------------ mutations exceed it
def _shifted(k, r, drop):
    """The coefficients task_coeff would return had it taken the split at k + 1 (``drop`` False) or k - 1: the fp16
    field beyond k is zero, the codes beyond r - k are zero (pack_small)."""
    def one(e, t):
        full = ap.coef(e, t)
        if not drop:      # k + 1: column k from c_high's zero padding, the low columns one code late
            return np.concatenate([full[:k], [np.float32(0)], full[k:r - 1]]).astype(np.float32)
        codes = np.concatenate([e.codes[t], np.zeros((e.stages, 1), np.uint8)], axis=1)
        low = ap.dequantize(codes, e.scale[t], e.zero_point[t])
        return np.concatenate([full[:k - 1], low]).astype(np.float32)
    return one


def _mutations(e, base):
    """{name: (applies, mutated [rows, N] fp64 or None)} for one parameter."""
    C = ap.coefs(e)
    want, _ = ap.task_rows(e, SCALE, base, C=C)
    idx = np.arange(e.rows)
    out = {"row dropped": (True, want[np.minimum(idx + 1, e.rows - 1)]),
           "row twice": (True, want[np.maximum(idx - 1, 0)])}
    k, r = e.k, e.r
    # a mutation of the coefficients applies where it changes a coefficient: a split moved over a code that equals its
    # zero point in every stage, or an omitted stage whose codes all do, reads the same numbers
    for name, ok, drop in (("split at k + 1", k < r, False), ("split at k - 1", k >= 1, True)):
        if ok:
            f = _shifted(k, r, drop)
            Cm = np.stack([f(e, t) for t in range(e.n)])
            out[name] = (not np.array_equal(Cm, C), ap.task_rows(e, SCALE, base, C=Cm)[0])
        else:
            out[name] = (False, None)
    less = np.stack([ap.coef(e, t, stages=range(e.stages - 1)) for t in range(e.n)])
    assert r > k or np.array_equal(less, C)
    out["a stage omitted"] = (not np.array_equal(less, C), ap.task_rows(e, SCALE, base, C=less)[0])
    sc = float(np.float32(SCALE))
    b = base.astype(np.float64)[:, None]
    y = e.U64 @ C.astype(np.float64).T
    out["mean omitted"] = (e.mean64 is not None, y * sc + b)
    out["scale before mean"] = (e.mean64 is not None, y * sc + (0.0 if e.mean64 is None else e.mean64[:, None]) + b)
    return want, out


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_mutation_exceeds_the_bound_on_a_spiked_row(case):
    """What a mutation cannot touch -- k = r has no low column to move or to omit a stage of, k = 0 no high column, an
    uncentred plan no mean -- is asserted too: there the mutated rows ARE the model's."""
    c = _contents(case)
    g = np.random.default_rng(case[0] + 100)
    seen = {}
    for p, e in c.live():
        base = g.standard_normal(e.rows).astype(np.float32)
        _, bound = ap.task_rows(e, SCALE, base)
        want, muts = _mutations(e, base)
        sp = ap.spike_rows(e.rows)
        for name, (applies, got) in muts.items():
            if got is None:
                assert not applies
                continue
            if not applies:
                assert np.array_equal(got, want), (name, p)
                continue
            if e.rows == 1 and name in ("row dropped", "row twice"):
                assert np.array_equal(got, want)      # one row: nothing to shift
                continue
            over = np.abs(got - want)[sp] > bound[sp]
            assert over.any(), (name, p, e.rows, e.k, e.r)
            seen[name] = seen.get(name, 0) + 1
    assert set(seen) == {"row dropped", "row twice", "split at k + 1", "split at k - 1", "a stage omitted"} | (
        {"mean omitted", "scale before mean"} if case[2] else set())


# ------------------------------------------------------------------------------------------------ the stores of part 4
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("T", [3, 8, 17, 20])
def test_store_magnitudes_have_no_threshold_ties_and_the_trim_bites(T, fp16):
    """The values of the dictionary-level stores (fp64 model, rounded to fp32): the TIES threshold of every task is
    reached by exactly one element, so the selection has no ties; most values are trimmed at density 0.2, signs
    conflict among the kept ones, and the spiked rows are the ones that survive."""
    c = ap.Contents(T, fp16=fp16, center=True, zero=False)
    v = np.concatenate([ap.task_rows(e)[0].T for _, e in c.live()], axis=1).astype(np.float32)
    assert np.isfinite(v).all()
    D = v.shape[1]
    tau = tm.thresholds(v, 0.2)
    assert ((np.abs(v) == tau[:, None]).sum(axis=1) == 1).all()
    _, ws = tm.ties_merge(v, 0.2)
    assert (ws["kept"] == D - tm.rank_of(D, 0.2) + 1).all()      # exactly the wanted count: nothing tied in
    assert (ws["kept"] < D).all() and ws["sign_conflict_rows"] > 0 and ws["empty_rows"] > 0
