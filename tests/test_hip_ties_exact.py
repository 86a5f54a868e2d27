"""
The TIES merge on a hand-built reference-layout store whose every value is an exact small integer: integer basis
columns, fp16-exact integer coefficients, an integer mean, no low part.  That gives what random data never does --
massive magnitude ties at the threshold (kept > keep_n, and exactly the model's count) and rows whose kept values cancel
exactly (s == 0 elects positive) -- and, with an fp16 and an fp32 basis group, two plans in one store, so the threshold
has to be global across plans: the same model with one threshold PER PLAN gives another result on this input, which the
test asserts so that it cannot pass by accident.
"""
import numpy as np
import pytest
import torch

import ties_model as tm

pytestmark = pytest.mark.gpu

TASKS = ["a", "b", "c", "d"]
SIZES = {"big.w": 5003, "small.w": 3001}      # big.w: several work units
NAMES = sorted(SIZES)
K = {"big.w": 3, "small.w": 2}


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _store():
    """Reference-layout dictionaries (CPU tensors) and the integer values they stand for, v [T, D] as int64."""
    g = torch.Generator().manual_seed(11)
    bases, comp, exact = {}, {n: {} for n in NAMES}, {}
    for n in NAMES:
        rows, k = SIZES[n], K[n]
        fp16 = n == "big.w"
        # big.w: entries up to 6 and a mean; small.w: entries up to 1, no mean -- its magnitudes are far smaller
        U = torch.randint(-6, 7, (rows, k), generator=g) if fp16 else torch.randint(-1, 2, (rows, k), generator=g)
        mean = torch.randint(-2, 3, (rows,), generator=g) if fp16 else None
        dt = torch.float16 if fp16 else torch.float32
        bases[n] = {"masked": {"U_high": U.to(dt), "U_low": torch.zeros(rows, 0, dtype=dt), "singular_values": torch.ones(k),
                               "k": k, "mean": mean.float() if mean is not None else None, "energy_retained": 1.0,
                               "D": rows, "N": len(TASKS)},
                    "noise": None}
        per = {}
        for i, t in enumerate(TASKS):
            # task b is minus task a (without the mean their values cancel exactly row by row)
            c = torch.randint(-3, 4, (k,), generator=g) if t != "b" else -per["a"]
            per[t] = c
            comp[n][t] = {"masked": {"c_high_fp16": c.to(torch.float16),
                                     "c_low_quant": {"payloads": [], "num_bits": 4, "num_stages": 2,
                                                     "original_shape": torch.Size([0]), "original_dtype": "torch.float32"}}}
        exact[n] = torch.stack([U @ per[t] + (mean if mean is not None else 0) for t in TASKS])
    return bases, comp, torch.cat([exact[n] for n in NAMES], dim=1).numpy()


def test_integer_store_ties_cancellation_and_a_global_threshold(sq):
    bases, comp, exact = _store()
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_low_bits=4, svd_rtvq_stages=2)
    shapes = {n: torch.Size([r]) for n, r in SIZES.items()}
    ab, ac = sq.adopt_artifacts(bases, comp, cfg, device="cuda")
    plans = {n: ab[n]["masked"]._batch[0].plan for n in NAMES}
    assert plans["big.w"] is not plans["small.w"] and plans["big.w"].fp16 and not plans["small.w"].fp16
    assert plans["big.w"].sizes.n_units > 1
    recon = sq.reconstruct_task_vectors(ac, ab, {}, shapes, cfg, device="cuda")
    v = tm.stack_values(recon, TASKS, NAMES, SIZES)
    assert np.array_equal(v.astype(np.int64), exact) and np.array_equal(v, exact.astype(np.float32))
    D = v.shape[1]
    g = torch.Generator().manual_seed(12)
    base = {n: torch.randint(-5, 6, s, generator=g).float().cuda() for n, s in shapes.items()}
    base_flat = tm.stack_values({"b": base}, ["b"], NAMES, SIZES)[0]
    for density in (0.2, 0.5, 1.0):
        for merge_func in ("mean", "sum"):
            got, stats = sq.ties_merge_parameters(ac, ab, shapes, cfg, density=density, scaling=0.5, merge_func=merge_func,
                                                  base_state_dict=base, device="cuda", return_stats=True)
            want, ws = tm.ties_merge(v, density, merge_func, 0.5, base_flat)
            flat = np.concatenate([got[n].cpu().numpy().reshape(-1) for n in NAMES])
            assert np.array_equal(flat.view(np.uint32), want.view(np.uint32)), (density, merge_func)
            assert [stats["thresholds"][t] for t in TASKS] == ws["thresholds"].tolist()
            assert [stats["kept"][t] for t in TASKS] == ws["kept"].tolist()
            assert (stats["sign_conflict_rows"], stats["empty_rows"]) == (ws["sign_conflict_rows"], ws["empty_rows"])
    # ---- what makes this input sharp, at density 0.2
    tau = tm.thresholds(v, 0.2)
    _, ws = tm.ties_merge(v, 0.2)
    keep_n = int(D * 0.2)
    at_tau = (np.abs(v) == tau[:, None]).sum(axis=1)
    assert (at_tau > 10).all() and (ws["kept"] > keep_n).all()      # ties at the threshold: more than keep_n are kept
    kept = np.abs(v) >= tau[:, None]
    s = np.where(kept, v, 0).sum(axis=0, dtype=np.float64)          # exact: small integers
    cancel = (s == 0) & (kept & (v > 0)).any(axis=0) & (kept & (v < 0)).any(axis=0)
    assert cancel.sum() > 10                                        # kept values that cancel exactly: positive is elected
    merged, _ = tm.ties_merge(v, 0.2, "sum")
    assert (merged[cancel] > 0).all()
    # a threshold per plan (each parameter group trimmed on its own) is another merge on this input
    per_plan = np.empty_like(v)
    off = 0
    for n in NAMES:
        per_plan[:, off:off + SIZES[n]] = tm.thresholds(v[:, off:off + SIZES[n]], 0.2)[:, None]
        off += SIZES[n]
    other, _ = tm.ties_merge(v, 0.2, "mean", tau=per_plan)
    mine, _ = tm.ties_merge(v, 0.2, "mean")
    assert not np.array_equal(other, mine)
    got = sq.ties_merge_parameters(ac, ab, shapes, cfg, density=0.2, device="cuda")
    flat = np.concatenate([got[n].cpu().numpy().reshape(-1) for n in NAMES])
    assert np.array_equal(flat.view(np.uint32), mine.view(np.uint32)) and not np.array_equal(flat, other)
