"""
GPU tests of the four store merges (TIES, DARE, TALL / consensus, EMR) away from k = 1: dictionary-level stores whose
parameters cover the (k, r) plane (tests/artifact_plane.py), adopted through driver.adopt_artifacts.

The chain is anchored first: what ``reconstruct_task_vectors`` returns on the adopted dictionaries is within the derived
bound of the fp64 model of the artifacts, element by element, and finite.  On those values the existing numpy models
hold the merges to bits.  The comparisons are those of test_hip_ties_merge.py, test_hip_dare_merge.py,
test_hip_tall_consensus.py and test_hip_emr_merge.py (``_check``, ``_grid``, ``_compare``), copied assertion for
assertion: theirs read their modules' parameter names, sizes and offsets, these take the store's.
"""
import numpy as np
import pytest
import torch

import artifact_plane as ap
import dare_model as dm
import emr_model as em
import tall_model as tlm
import ties_model as tm
import test_hip_dare_merge as t_dare
import test_hip_emr_merge as t_emr
import test_hip_tall_consensus as t_tall

pytestmark = pytest.mark.gpu

CASES = [(T, fp16) for T in (3, 8, 17, 20) for fp16 in (True, False)]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Store:
    """One adopted store and the values it reconstructs; shared and left unchanged."""

    def __init__(self, sq, T, fp16):
        self.c = c = ap.Contents(T, fp16=fp16, center=True, zero=False)
        self.names, self.tasks, bases, comp = c.dictionaries()
        self.sizes = {n: e.rows for n, (_, e) in zip(self.names, c.live())}
        self.D = sum(self.sizes.values())
        self.off, pos = {}, 0
        for n in self.names:
            self.off[n] = pos
            pos += self.sizes[n]
        self.n_bytes = (self.D + 7) // 8
        self.cfg = sq.SVDHybridConfig(tasks=self.tasks, svd_low_bits=c.bits, svd_rtvq_stages=c.stages, svd_fp16=fp16,
                                      svd_center=True)
        self.bases, self.comp = sq.adopt_artifacts(bases, comp, self.cfg, device="cuda")
        # nothing was declined: every parameter came back backed by a plan, and it is one plan
        assert all(getattr(self.bases[n]["masked"], "_batch", None) is not None for n in self.names)
        assert all(getattr(self.comp[n], "_batch", None) is not None for n in self.names)
        plans = {id(self.bases[n]["masked"]._batch[0].plan) for n in self.names}
        assert len(plans) == 1
        self.plan = self.bases[self.names[0]]["masked"]._batch[0].plan
        assert self.plan.N == T and self.plan.fp16 == fp16 and self.plan.center and self.plan.P == len(self.names)
        self.shapes = {n: torch.Size([r]) for n, r in self.sizes.items()}
        recon = sq.reconstruct_task_vectors(self.comp, self.bases, {}, self.shapes, self.cfg, device="cuda")
        self.v, self.has = dm.stack_values(recon, self.tasks, self.names, self.sizes)
        assert self.has.all() and np.isfinite(self.v).all()
        assert np.array_equal(self.v, tm.stack_values(recon, self.tasks, self.names, self.sizes))
        g = torch.Generator().manual_seed(7 + T)
        self.base = {n: torch.randn(s, generator=g).cuda() for n, s in self.shapes.items()}
        self.base_flat = tm.stack_values({"b": self.base}, ["b"], self.names, self.sizes)[0]


_STORES = {}


def _store(sq, T, fp16):
    if (T, fp16) not in _STORES:
        _STORES[(T, fp16)] = _Store(sq, T, fp16)
    return _STORES[(T, fp16)]


# ------------------------------------------------------------------------------------------ the anchor
@pytest.mark.parametrize("T,fp16", CASES)
def test_store_values_are_within_the_bound_of_fp64(sq, T, fp16):
    st = _store(sq, T, fp16)
    ks = {e.k for _, e in st.c.live()}
    assert max(ks) >= min(T, 8) - 1 and {k % 2 for k in ks} == {0, 1}      # far from k = 1
    for n, (p, e) in zip(st.names, st.c.live()):
        want, bound = ap.task_rows(e)
        got = st.v[:, st.off[n]:st.off[n] + e.rows].T.astype(np.float64)
        err = np.abs(got - want)
        assert (err <= bound).all(), (n, float((err / bound).max()))


# ------------------------------------------------------------------------------------------ TIES
def _check_ties(sq, st, density, merge_func, scaling, with_base):
    """test_hip_ties_merge.py's _check: merged tensors and thresholds bit for bit, kept counts and row counters equal."""
    order, v = st.tasks, st.v
    got, stats = sq.ties_merge_parameters(st.comp, st.bases, st.shapes, st.cfg, density=density, scaling=scaling,
                                          merge_func=merge_func, base_state_dict=st.base if with_base else None,
                                          device="cuda", return_stats=True)
    want, ws = tm.ties_merge(v, density, merge_func, scaling, st.base_flat if with_base else None)
    what = (len(order), density, merge_func, scaling, with_base)
    assert sorted(got) == st.names, what
    want_by = tm.split_rows(want, st.names, st.sizes)
    for n in st.names:
        assert got[n].is_cuda and got[n].shape == st.shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    assert list(stats["thresholds"]) == list(order) and list(stats["kept"]) == list(order), what
    tau = np.array([stats["thresholds"][t] for t in order], dtype=np.float32)
    assert _same_bits(tau, ws["thresholds"]), (what, tau, ws["thresholds"])
    assert [stats["kept"][t] for t in order] == ws["kept"].tolist(), what
    assert stats["sign_conflict_rows"] == ws["sign_conflict_rows"] and stats["empty_rows"] == ws["empty_rows"], what
    assert stats["rows"] == st.D
    return stats, ws


@pytest.mark.parametrize("T,fp16", CASES)
def test_ties_merge_matches_the_model_bit_for_bit(sq, T, fp16):
    st = _store(sq, T, fp16)
    for density in (0.2, 1.0):
        for merge_func in ("mean", "sum"):
            for with_base in (False, True):
                scaling = 0.3 if (with_base or merge_func == "sum") else 1.0
                stats, ws = _check_ties(sq, st, density, merge_func, scaling, with_base)
                assert all(c >= max(int(st.D * density), 1) for c in ws["kept"])
    # the trim does something here, signs conflict among the kept values, and no magnitude ties at a threshold
    _, ws = tm.ties_merge(st.v, 0.2)
    assert ws["sign_conflict_rows"] > 0 and (ws["kept"] < st.D).all()
    assert (ws["kept"] == st.D - tm.rank_of(st.D, 0.2) + 1).all()


# ------------------------------------------------------------------------------------------ DARE
def _check_dare(sq, st, words, drop_rate, rescale, weights, normalize, scaling, with_base, seed=t_dare.SEED):
    """test_hip_dare_merge.py's _check: merged tensors bit for bit, kept counts equal."""
    order = st.tasks
    wd = None if weights is None else dict(zip(order, weights))
    got, stats = sq.dare_merge_parameters(st.comp, st.bases, st.shapes, st.cfg, drop_rate=drop_rate, seed=seed,
                                          rescale=rescale, weights=wd, normalize=normalize, scaling=scaling,
                                          base_state_dict=st.base if with_base else None, device="cuda",
                                          return_stats=True)
    want, ws = dm.dare_merge(st.v, st.has, drop_rate, seed, rescale, weights, normalize, scaling,
                             st.base_flat if with_base else None, all_words=words)
    what = (len(order), drop_rate, rescale, weights is not None, normalize, scaling, with_base)
    assert sorted(got) == st.names, what
    want_by = dm.split_rows(want, st.names, st.sizes)
    for n in st.names:
        assert got[n].is_cuda and got[n].shape == st.shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    assert list(stats["kept"]) == list(order), what
    assert [stats["kept"][t] for t in order] == ws["kept"].tolist(), what
    assert stats["rows"] == st.D and stats["drop_threshold"] == ws["drop_threshold"] == dm.drop_threshold(drop_rate), what
    return stats, ws


@pytest.mark.parametrize("T,fp16", CASES)
def test_dare_merge_matches_the_model_bit_for_bit(sq, T, fp16):
    """That file's grid: every drop rate x rescale x weights x base."""
    st = _store(sq, T, fp16)
    words = dm.words(T, st.D, t_dare.SEED)
    kept = {}
    for drop_rate in t_dare.DROP_RATES:
        for rescale in (True, False):
            for weights in (None, t_dare._given_weights(T)):
                for with_base in (False, True):
                    _, ws = _check_dare(sq, st, words, drop_rate, rescale, weights, False, 0.3 if with_base else 1.0,
                                        with_base)
                    kept[drop_rate] = ws["kept"]
    D = st.D
    assert (kept[0.0] == D).all()
    for p in t_dare.DROP_RATES[1:]:
        assert (np.abs(kept[p] - D * (1 - p)) <= 6 * np.sqrt(D * p * (1 - p))).all(), (p, kept[p])
    _check_dare(sq, st, words, 0.9, True, [abs(w) for w in t_dare._given_weights(T)], True, 0.3, True)


# ------------------------------------------------------------------------------------------ TALL / consensus
def _check_tall(sq, st, lam, k, scaling, with_base):
    """test_hip_tall_consensus.py's _check: one combined call (merge + masks + stats) against the model."""
    order = st.tasks
    arg = dict(zip(order, lam)) if isinstance(lam, list) else lam
    got, masks, stats = sq.consensus_merge_parameters(st.comp, st.bases, st.shapes, st.cfg, tall_lambda=arg, k=k,
                                                      scaling=scaling, base_state_dict=st.base if with_base else None,
                                                      return_masks=True, device="cuda", return_stats=True)
    want, wm, ws = tlm.consensus_merge(st.v, st.has, lam, k, scaling, st.base_flat if with_base else None)
    what = (len(order), lam if not isinstance(lam, list) else "per task", k, scaling, with_base)
    assert sorted(got) == st.names, what
    want_by = tlm.split_rows(want, st.names, st.sizes)
    for n in st.names:
        assert got[n].is_cuda and got[n].shape == st.shapes[n] and got[n].dtype is torch.float32, (what, n)
        assert _same_bits(got[n].cpu().numpy(), want_by[n]), (what, n)
    streams = tlm.pack_streams(tlm.split_rows(wm, st.names, st.sizes), st.off, st.D)
    assert list(masks) == list(order), what
    for g, t in enumerate(order):
        assert masks[t].is_cuda and masks[t].dtype is torch.uint8 and masks[t].shape == (st.n_bytes,), (what, t)
        assert np.array_equal(masks[t].cpu().numpy(), streams[g]), (what, t)
    assert list(stats["active"]) == list(order), what
    assert [stats["active"][t] for t in order] == ws["active"].tolist(), what
    assert stats["agreement"] == ws["agreement"].tolist() and sum(stats["agreement"]) == st.D, what
    assert stats["rows"] == st.D == ws["rows"], what
    return masks, wm, ws


@pytest.mark.parametrize("T,fp16", CASES)
def test_consensus_merge_and_tall_masks_match_the_model(sq, T, fp16):
    """That file's grid: lambda {0, middle, per task} x k {0, 1, 2, T} x base / no base."""
    st = _store(sq, T, fp16)
    mid = None
    for lam in (0.0, t_tall._middle(T), t_tall._per_task(T)):
        for k in sorted({0, 1, min(2, T), T}):
            for with_base in (False, True):
                _, wm, ws = _check_tall(sq, st, lam, k, 0.3 if with_base else 1.0, with_base)
                if lam == t_tall._middle(T):
                    mid = (wm, ws)
    t_tall._assert_not_vacuous(mid[0], mid[1], st.has, T)
    # the mask-only call gives the streams of the combined call, which the model pinned
    lam = t_tall._per_task(T)
    masks, _, _ = _check_tall(sq, st, lam, 2, 1.0, False)
    only, stats = sq.tall_masks_from_store(st.comp, st.bases, st.shapes, st.cfg, tall_lambda=dict(zip(st.tasks, lam)),
                                           device="cuda", return_stats=True)
    assert list(only) == st.tasks and stats["rows"] == st.D
    for t in st.tasks:
        assert torch.equal(only[t], masks[t]), t


# ------------------------------------------------------------------------------------------ EMR
def _emr_not_vacuous(model, st):
    """test_hip_emr_merge.py's _assert_not_vacuous on the model's output alone, asked of EVERY parameter of 64 rows or
    more: every task's mask is neither empty nor full and the largest magnitude loses the election somewhere.  Where it
    does not hold the parameter must have r <= 2 -- it spans two directions, so its tasks may agree in sign on every
    row -- and nothing else is excused: from r = 3 on there is no exception, and most parameters are of that kind."""
    v, T = st.v, st.v.shape[0]
    top = np.abs(v).max(axis=0)
    excused, asked = [], 0
    for n, (_, e) in zip(st.names, st.c.live()):
        if st.sizes[n] < 64:
            continue
        asked += 1
        rows = slice(st.off[n], st.off[n] + st.sizes[n])
        problems = []
        for g in range(T):
            if not (model["masks"][g, rows].any() and not model["masks"][g, rows].all()):
                problems.append(f"{n}: the mask of task {g} is {'full' if model['masks'][g, rows].all() else 'empty'}")
        if not (np.abs(model["tau"][rows]) < top[rows]).any():
            problems.append(f"{n}: every row elects its largest magnitude")
        assert not problems or e.r <= 2, problems
        if problems:
            excused.append(n)
    assert len(set(model["lambda"].tolist())) > 1, "the rescalers are all equal"
    assert asked >= 20 and len(excused) <= asked // 5, (asked, excused)


def _compare_emr(got, model, st, what=""):
    """test_hip_emr_merge.py's _compare: the four results of one emr_merge_parameters call against the model."""
    order, has, total = st.tasks, st.has, st.D
    unified, masks, rescalers, stats = got
    assert sorted(unified) == st.names, what
    for n, x in tlm.split_rows(model["tau"], st.names, st.sizes).items():
        assert unified[n].is_cuda and unified[n].dtype is torch.float32 and tuple(unified[n].shape) == (st.sizes[n],), (what, n)
        assert np.array_equal(t_emr._u32(unified[n].cpu().numpy()), t_emr._u32(x)), (what, n)
    streams = tlm.pack_streams(tlm.split_rows(model["masks"], st.names, st.sizes), st.off, total)
    assert list(masks) == list(order) == list(rescalers), what
    for g, t in enumerate(order):
        assert masks[t].is_cuda and masks[t].dtype is torch.uint8 and masks[t].shape == ((total + 7) // 8,), (what, t)
        assert np.array_equal(masks[t].cpu().numpy(), streams[g]), (what, t)
    assert stats["rows"] == st.D and list(stats["active"]) == list(order), what
    assert [stats["active"][t] for t in order] == model["masks"].sum(axis=1).tolist(), what
    for g, t in enumerate(order):
        n = int(has[g].sum())
        t_emr._close(stats["abs_sum"][t], float(model["A"][g]), n, f"{what} A[{t}]")
        t_emr._close(stats["masked_sum"][t], float(model["B"][g]), n, f"{what} B[{t}]")
        a, b = stats["abs_sum"][t], stats["masked_sum"][t]
        assert rescalers[t] == (a / b if b != 0.0 else 1.0), (what, t)      # the fp64 quotient of the two sums
        assert abs(rescalers[t] - model["lambda"][g]) <= 3 * n * t_emr.REL * model["lambda"][g], (what, t)


@pytest.mark.parametrize("T,fp16", CASES)
def test_emr_merge_and_task_models_match_the_model(sq, T, fp16):
    st = _store(sq, T, fp16)
    model = em.emr_merge(st.v, st.has)
    _emr_not_vacuous(model, st)
    got = sq.emr_merge_parameters(st.comp, st.bases, st.shapes, st.cfg, device="cuda", return_stats=True)
    _compare_emr(got, model, st, what=f"T = {T}, fp16 {fp16}")
    unified, masks, rescalers, _ = got
    for g, t in enumerate(st.tasks):
        for b, flat in ((None, None), (st.base, st.base_flat)):
            out = sq.emr_task_state_dict(unified, masks, rescalers, t, base_state_dict=b, device="cuda")
            want = em.task_model(model["tau"], model["masks"][g], rescalers[t], flat)
            assert sorted(out) == sorted(st.names)
            for n, x in tlm.split_rows(want, st.names, st.sizes).items():
                assert np.array_equal(t_emr._u32(out[n].cpu().numpy()), t_emr._u32(x)), (t, n, b is not None)
