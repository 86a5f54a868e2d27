"""
The Model Breadcrumbs merge on a hand-built reference-layout store whose every value is an exact integer, adopted into
two plans (an fp16 basis group with a mean, an fp32 one without).  The magnitudes are chosen so that the two thresholds of
a (parameter, task) part ways at each of the four radix digits in turn:

    big.w   small integers (|v| <= 56): at the defaults lo = 2 and hi >= 27 differ in the top byte      -> digit 0
    f1.w    +-(2^20 + 2^13 j), 7 <= j <= 65: same exponent, mantissa bits 22 .. 16 differ      -> digit 1
    f2.w    +-(2^20 + 2^5 j): mantissa bits 12 .. 5 differ                                     -> digit 2
    m3.w    2^20 + 16 + x, |x| <= 9: mantissa bits 7 .. 3 differ                               -> digit 3
    tiny.w  4 rows: n_keep == 0 at density 0.2 beside the full bands of its plan; lo == hi at (0.25, 0.25)

Integer values give what random data never does: massive ties at both thresholds (kept > n_keep, and exactly the model's
count), lo == hi, and -- task b is minus task a in the group without a mean, so their bands are equal -- rows whose kept
values cancel exactly (s == 0 elects positive).  The last part shows that the per-tensor thresholds are not the global
threshold ``ties_merge_parameters`` finds on the same store.
"""
import numpy as np
import pytest
import torch

import breadcrumbs_model as bm
import ties_model as tm

pytestmark = pytest.mark.gpu

TASKS = ["a", "b", "c", "d"]
SIZES = {"big.w": 5003, "f1.w": 3001, "f2.w": 2049, "m3.w": 1300, "tiny.w": 4}      # big.w: several work units
NAMES = sorted(SIZES)
BOUNDS = np.concatenate([[0], np.cumsum([SIZES[n] for n in NAMES])])
FP16 = ("big.w", "m3.w", "tiny.w")
PAIRS = ((0.2, 0.0), (0.5, 0.1), (0.25, 0.25), (0.9, 0.01), (1.0, 0.0))


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _store():
    """Reference-layout dictionaries (CPU tensors) and the integer values they stand for, v [T, D] as int64."""
    g = torch.Generator().manual_seed(21)
    bases, comp, exact = {}, {n: {} for n in NAMES}, {}

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g)

    for n in NAMES:
        rows = SIZES[n]
        fp16 = n in FP16
        if n in ("big.w", "tiny.w"):
            U, mean = ri(-6, 6, rows, 3), ri(-2, 2, rows)
            coeff = {t: ri(-3, 3, 3) for t in TASKS}
        elif n == "m3.w":
            U, mean = ri(-1, 1, rows, 3), torch.full((rows,), (1 << 20) + 16)
            coeff = {t: ri(-3, 3, 3) for t in TASKS}
        else:
            step = 1 << (13 if n == "f1.w" else 5)
            U = torch.stack([(1 << 20) + step * ri(16, 56, rows), step * ri(0, 3, rows)], dim=1)
            mean = None
            coeff = {"a": torch.tensor([1, int(ri(-3, 3, 1))]), "c": torch.tensor([1, int(ri(-3, 3, 1))]),
                     "d": torch.tensor([-1, int(ri(-3, 3, 1))])}
            coeff["b"] = -coeff["a"]      # the values of a and b cancel exactly, row by row
        dt = torch.float16 if fp16 else torch.float32
        k = U.shape[1]
        bases[n] = {"masked": {"U_high": U.to(dt), "U_low": torch.zeros(rows, 0, dtype=dt), "singular_values": torch.ones(k),
                               "k": k, "mean": mean.float() if mean is not None else None, "energy_retained": 1.0,
                               "D": rows, "N": len(TASKS)},
                    "noise": None}
        for t in TASKS:
            comp[n][t] = {"masked": {"c_high_fp16": coeff[t].to(torch.float16),
                                     "c_low_quant": {"payloads": [], "num_bits": 4, "num_stages": 2,
                                                     "original_shape": torch.Size([0]), "original_dtype": "torch.float32"}}}
        exact[n] = torch.stack([U @ coeff[t] + (mean if mean is not None else 0) for t in TASKS])
    return bases, comp, torch.cat([exact[n] for n in NAMES], dim=1).numpy()


def _first_digit_apart(lo, hi):
    """The radix digit (0 = the top byte) at which the bit patterns of lo and hi first differ; None where lo == hi."""
    x = int(np.float32(lo).view(np.uint32)) ^ int(np.float32(hi).view(np.uint32))
    return None if x == 0 else next(d for d in range(4) if (x >> (24 - 8 * d)) & 0xff)


def test_integer_store_every_digit_ties_cancellation_and_an_empty_band(sq):
    bases, comp, exact = _store()
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_low_bits=4, svd_rtvq_stages=2)
    shapes = {n: torch.Size([r]) for n, r in SIZES.items()}
    ab, ac = sq.adopt_artifacts(bases, comp, cfg, device="cuda")
    plans = {n: ab[n]["masked"]._batch[0].plan for n in NAMES}
    assert len({id(p) for p in plans.values()}) == 2
    assert all(plans[n] is plans["big.w"] and plans[n].fp16 for n in FP16)
    assert plans["f1.w"] is plans["f2.w"] and not plans["f1.w"].fp16
    assert plans["big.w"].sizes.n_units > plans["big.w"].P
    recon = sq.reconstruct_task_vectors(ac, ab, {}, shapes, cfg, device="cuda")
    v = tm.stack_values(recon, TASKS, NAMES, SIZES)
    assert np.array_equal(v.astype(np.int64), exact) and np.array_equal(v, exact.astype(np.float32))
    g = torch.Generator().manual_seed(12)
    base = {n: torch.randint(-5, 6, s, generator=g).float().cuda() for n, s in shapes.items()}
    base_flat = tm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0]
    present = [[True] * len(TASKS) for _ in NAMES]
    seen = {}
    for density, gamma in PAIRS:
        banded = bm.bands(v, BOUNDS, present, density, gamma)
        for sign_election in (False, True):
            for merge_func in ("sum", "mean"):
                got, stats = sq.breadcrumbs_merge_parameters(ac, ab, shapes, cfg, density=density, gamma=gamma,
                                                             scaling=0.5, sign_election=sign_election,
                                                             merge_func=merge_func, base_state_dict=base, device="cuda",
                                                             return_stats=True)
                want, ws = bm.breadcrumbs_merge(v, BOUNDS, present, density, gamma, 0.5, sign_election, merge_func,
                                                base_flat, banded=banded)
                what = (density, gamma, sign_election, merge_func)
                flat = np.concatenate([got[n].cpu().numpy().reshape(-1) for n in NAMES])
                assert np.array_equal(flat.view(np.uint32), want.view(np.uint32)), what
                for p, n in enumerate(NAMES):
                    for g_, t in enumerate(TASKS):
                        wlh = ws["thresholds"][p][g_]
                        assert stats["thresholds"][n][t] == (None if wlh is None else (float(wlh[0]), float(wlh[1]))), what
                        assert stats["kept"][n][t] == ws["kept"][p, g_], (what, n, t)
                assert (stats["sign_conflict_rows"], stats["empty_rows"]) == (ws["sign_conflict_rows"], ws["empty_rows"])
        seen[density, gamma] = (banded, ws)
    # ---- what makes this input sharp
    # every digit is the first at which some (parameter, task)'s two thresholds part ways
    def apart(pair):
        ths = seen[pair][1]["thresholds"]
        return {n: {_first_digit_apart(*ths[p][g_]) for g_ in range(len(TASKS))} for p, n in enumerate(NAMES)}
    assert apart((0.9, 0.01))["big.w"] == {0}      # lo = 2, hi between 27 and 42: two octaves apart or more
    mid = apart((0.5, 0.1))
    assert mid["big.w"] == {1} and mid["f1.w"] == {1} and mid["f2.w"] == {2} and mid["m3.w"] == {3}, mid
    # ties at both thresholds: more than n_keep are kept, on every task of the small-integer tensor
    kept, ths = seen[0.5, 0.1]
    p = NAMES.index("big.w")
    seg = np.abs(v[:, BOUNDS[p]:BOUNDS[p + 1]])
    for g_ in range(len(TASKS)):
        lo, hi = ths["thresholds"][p][g_]
        assert (seg[g_] == lo).sum() > 10 and (seg[g_] == hi).sum() > 10
        assert ths["kept"][p, g_] > bm.counts(SIZES["big.w"], 0.5, 0.1)[0]
    # n_keep == 0 beside full bands of the same plan; lo == hi
    tiny = NAMES.index("tiny.w")
    assert bm.counts(4, 0.2, 0.0)[0] == 0 and not seen[0.2, 0.0][1]["kept"][tiny].any()
    assert all(th is None for th in seen[0.2, 0.0][1]["thresholds"][tiny])
    assert seen[0.2, 0.0][1]["kept"][p].min() >= int(5003 * 0.2)
    assert bm.counts(4, 0.25, 0.25) == (1, 1, 2)
    assert all(th[0] == th[1] for th in seen[0.25, 0.25][1]["thresholds"][tiny])
    # exact cancellation under election: a and b kept and opposite, nothing else kept -> s == 0 elects positive
    kept = seen[0.5, 0.1][0][0]
    f1 = slice(int(BOUNDS[NAMES.index("f1.w")]), int(BOUNDS[NAMES.index("f1.w") + 1]))
    s = np.where(kept, v, 0).sum(axis=0, dtype=np.float64)      # exact: integers below 2^24
    cancel = np.zeros(v.shape[1], dtype=bool)
    cancel[f1] = ((s == 0) & (kept & (v > 0)).any(axis=0) & (kept & (v < 0)).any(axis=0))[f1]
    assert cancel.sum() > 10
    merged, _ = bm.breadcrumbs_merge(v, BOUNDS, present, 0.5, 0.1, 1.0, True, "sum")
    assert (merged[cancel] > 0).all()


def test_per_tensor_thresholds_are_not_the_global_threshold(sq):
    bases, comp, exact = _store()
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_low_bits=4, svd_rtvq_stages=2)
    shapes = {n: torch.Size([r]) for n, r in SIZES.items()}
    ab, ac = sq.adopt_artifacts(bases, comp, cfg, device="cuda")
    glob, gs = sq.ties_merge_parameters(ac, ab, shapes, cfg, density=0.2, device="cuda", return_stats=True)
    per, ps = sq.breadcrumbs_merge_parameters(ac, ab, shapes, cfg, density=0.2, gamma=0.0, sign_election=True,
                                              merge_func="mean", device="cuda", return_stats=True)
    # the global trim spends its whole budget on the tensors of magnitude 2^20: nothing of big.w survives it, while
    # the per-tensor trim keeps a fifth of every tensor that has five rows or more
    for t in TASKS:
        assert gs["thresholds"][t] >= 2.0 ** 20
        assert ps["thresholds"]["big.w"][t][0] < 64 and ps["kept"]["big.w"][t] >= int(5003 * 0.2)
        assert ps["thresholds"]["f1.w"][t][0] >= 2.0 ** 20
    assert not glob["big.w"].any() and per["big.w"].any()
    # and where every tensor is kept whole the two operators agree bit for bit (same election, same mean)
    glob, _ = sq.ties_merge_parameters(ac, ab, shapes, cfg, density=1.0, device="cuda", return_stats=True)
    per = sq.breadcrumbs_merge_parameters(ac, ab, shapes, cfg, density=1.0, gamma=0.0, sign_election=True,
                                          merge_func="mean", device="cuda")
    for n in NAMES:
        assert torch.equal(glob[n].view(torch.int32), per[n].view(torch.int32)), n
