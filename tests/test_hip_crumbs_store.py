"""
The Model Breadcrumbs merge from a saved store (storage.breadcrumbs_merge_from_artifacts, scripts/breadcrumbs_merge.py):
the same bits as the dictionary route on the fused run that wrote the store, the store's files untouched; the launches
counted per plan (one histogram launch per digit up to 16 tasks, two above); the refusals name the parameter; the
footprint is the output plus the state table plus small tables; and no task model is reconstructed on the way.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (130, 64), "head.w": (257, 33)}
TASKS = ["A", "B", "C", "D", "E", "F"]
CRUMBS = ("svdq_plan_crumbs_hist", "svdq_plan_crumbs_select_step", "svdq_plan_crumbs_merge")
NEVER = ("svdq_task_reconstruct", "svdq_reconstruct")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().contiguous().view(torch.int32),
                                                                     b.cpu().contiguous().view(torch.int32))


def _digest(d):
    return {f: hashlib.sha256(open(os.path.join(r, f), "rb").read()).hexdigest()
            for r, _, fs in os.walk(d) for f in fs}


class _Spy:
    """Counters on the library's own entry points."""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls = lib, names, dict.fromkeys(names, 0)

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in self.names}
        for n in self.names:
            setattr(self.lib, n, self._wrap(n))
        return self.calls

    def _wrap(self, n):
        def call(*a):
            self.calls[n] += 1
            return self.real[n](*a)
        return call

    def __exit__(self, *exc):
        for n in self.names:
            setattr(self.lib, n, self.real[n])


@pytest.fixture(scope="module")
def store(sq, tmp_path_factory):
    """A fused run of six tasks over four parameters (task F lacks one), its store on disk and a base checkpoint with
    one key the store does not cover."""
    from oracle import svd_hybrid_oracle as orc
    tmp = tmp_path_factory.mktemp("crumbs_store")
    tv = {t: {} for t in TASKS}
    for pi, (n, shp) in enumerate(sorted(SHAPES.items())):
        for t, x in zip(TASKS, orc.synthetic_deltas(int(np.prod(shp)), len(TASKS), 900 + pi)):
            tv[t][n] = x.view(shp).cuda()
    del tv["F"]["enc/w2"]
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_energy_threshold=0.9, svd_max_rank=3, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    d = str(tmp / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()}},
                          cfg, d)
    g = torch.Generator().manual_seed(4)
    base = {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}
    base["head.bias"] = torch.randn(10, generator=g)
    torch.save(base, str(tmp / "base.pt"))
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    return cfg, bases, comp, shapes, d, base, str(tmp)


def test_store_and_script_equal_the_dictionary_route(sq, store):
    cfg, bases, comp, shapes, d, base, tmp = store
    kw = dict(density=0.6, gamma=0.05, scaling=0.7, sign_election=True, merge_func="mean")
    dev_base = {n: b.cuda() for n, b in base.items() if n in shapes}
    want, wstats = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, base_state_dict=dev_base, device="cuda",
                                                   return_stats=True, **kw)
    before = _digest(d)
    out_path = os.path.join(tmp, "merged_api.pt")
    with _Spy(sq._native.lib(), CRUMBS + NEVER) as calls:
        res = sq.breadcrumbs_merge_from_artifacts(d, os.path.join(tmp, "base.pt"), out_path, device="cuda", **kw)
    # task F lacks a parameter: adoption makes two plans, each with its own table: 4 digits, one merge
    assert calls == {"svdq_plan_crumbs_hist": 8, "svdq_plan_crumbs_select_step": 8, "svdq_plan_crumbs_merge": 2,
                     "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}, calls
    assert _digest(d) == before
    merged = res["merged_state_dict"]
    assert sorted(merged) == sorted(base)
    for n in shapes:
        assert merged[n].shape == shapes[n] and _bits(merged[n], want[n]), n
    assert _bits(merged["head.bias"], base["head.bias"])
    assert res["stats"] == wstats and res["stats"]["rows"] == sum(int(np.prod(s)) for s in SHAPES.values())
    assert sorted(res["stats"]["thresholds"]) == sorted(SHAPES) and sorted(res["stats"]["kept_total"]) == TASKS
    assert list(res["stats"]["thresholds"]["enc/w2"]) == TASKS[:5] and "F" in res["stats"]["thresholds"]["head.w"]
    saved = torch.load(out_path, weights_only=True)
    assert sorted(saved) == sorted(base) and all(_bits(saved[n], merged[n]) for n in saved)
    # ---- the script, with a subset of tasks, the paper's combination and the outlier cut off
    want2, wstats2 = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, density=0.5, gamma=0.0, scaling=1.0,
                                                     tasks=["B", "F", "D"], base_state_dict=dev_base, device="cuda",
                                                     return_stats=True)
    script_out = os.path.join(tmp, "merged_script.pt")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "breadcrumbs_merge.py"), "--artifact-dir", d,
                         "--base-model-path", os.path.join(tmp, "base.pt"), "--output-path", script_out, "--density", "0.5",
                         "--gamma", "0", "--merge-func", "sum", "--tasks", "B", "F", "D"], capture_output=True, text=True,
                        timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [json.loads(ln) for ln in rc.stdout.splitlines() if ln.startswith("{")]
    assert lines[0] == {"kept_total": wstats2["kept_total"]} and list(lines[0]["kept_total"]) == ["B", "D", "F"]
    assert lines[1] == {"sign_conflict_rows": wstats2["sign_conflict_rows"], "empty_rows": wstats2["empty_rows"],
                        "rows": wstats2["rows"]}
    saved = torch.load(script_out, weights_only=True)
    assert sorted(saved) == sorted(base)
    for n in shapes:
        assert _bits(saved[n], want2[n]), n
    assert _digest(d) == before
    with pytest.raises(ValueError, match="Z"):
        sq.breadcrumbs_merge_from_artifacts(d, base, tasks=["A", "Z"], device="cuda")


def test_two_calls_give_identical_bits(sq, store):
    cfg, bases, comp, shapes, d, base, tmp = store
    one, s1 = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    two, s2 = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    assert s1 == s2 and all(_bits(one[n], two[n]) and one[n].data_ptr() != two[n].data_ptr() for n in shapes)


def test_a_masked_store_and_a_declined_parameter_are_refused_by_name(sq, store, tmp_path):
    from oracle import svd_hybrid_oracle as orc
    cfg, bases, comp, shapes, d, base, tmp = store
    who = "breadcrumbs_merge_parameters"
    # ---- a parameter adoption declines (a basis dtype no plan holds) stays a plain dictionary
    art = sq.load_all_artifacts(d, device="cpu")
    art["bases"]["enc.b1"]["masked"]["U_high"] = art["bases"]["enc.b1"]["masked"]["U_high"].double()
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    with pytest.raises(ValueError, match=rf"{who}: parameter 'enc\.b1' is not backed by a plan"):
        sq.breadcrumbs_merge_parameters(ac, ab, shapes, cfg, device="cuda")
    # ---- a masked run's store holds the selected rows only
    tasks = TASKS[:4]
    g = torch.Generator().manual_seed(9)
    tv = {t: {"m.w": x.cuda()} for t, x in zip(tasks, orc.synthetic_deltas(4097, 4, 5))}
    masks = {"m.w": (torch.rand(4097, generator=g) < 0.6).cuda()}
    mcfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2,
                              svd_min_mask_size=10)
    mb, mc = sq.run_basis_and_compress(tv, masks, mcfg, "cuda")
    with pytest.raises(ValueError, match=rf"{who}: parameter 'm\.w'.*masked run"):
        sq.breadcrumbs_merge_parameters(mc, mb, {"m.w": torch.Size([4097])}, mcfg, device="cuda")
    md = str(tmp_path / "masked")
    sq.save_all_artifacts(mb, mc, {"per_parameter": {"m.w": {"original_shape": [4097]}}}, mcfg, md)
    with pytest.raises(ValueError, match=r"'m\.w'.*masked run"):
        sq.breadcrumbs_merge_from_artifacts(md, {"m.w": torch.zeros(4097)}, device="cuda")


def _one_parameter_store(sq, D, T):
    tasks = [f"t{i:02d}" for i in range(T)]
    g = torch.Generator(device="cuda").manual_seed(2)
    B = torch.randn(D, 3, generator=g, device="cuda")
    tv = {t: {"w": 0.01 * (B @ torch.randn(3, generator=g, device="cuda")) + 0.002 * torch.randn(D, generator=g, device="cuda")}
          for t in tasks}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    return cfg, bases, comp, {"w": torch.Size([D])}


@pytest.mark.parametrize("T,hists", [(8, 4), (16, 4), (17, 8)])
def test_launch_counts_and_footprint(sq, T, hists):
    """One parameter of 2^20 rows.  Up to 16 tasks one histogram launch per digit counts both bounds; above, two.  The
    rise of the peak during the merge is the output plus the state table plus the small tables (slot tables, ranks,
    pointer tables, the coefficients of the live tasks: well under 64 KB here) -- nothing proportional to D * T, where
    reconstruct_task_vectors for all tasks holds T x 4 D bytes."""
    D = 1 << 20
    cfg, bases, comp, shapes = _one_parameter_store(sq, D, T)
    plan = bases["w"]["masked"]._batch[0].plan
    table = int(sq._native.lib().svdq_crumbs_work_bytes(plan.P, T))
    assert table == 256 * -(-8 * (261 * plan.P * T + 2) // 256)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with _Spy(sq._native.lib(), CRUMBS + NEVER) as calls:
        got, stats = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"T {T}: peak rise {rise} bytes = output {4 * D} + table {table} + {rise - 4 * D - table}")
    assert rise <= 4 * D + table + (64 << 10), (rise, table)
    assert calls == {"svdq_plan_crumbs_hist": hists, "svdq_plan_crumbs_select_step": 4, "svdq_plan_crumbs_merge": 1,
                     "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}, calls
    # exact selection: n_keep = int(0.9 D) values and a few more where magnitudes tie at a threshold
    n_keep = int(D * 0.9)
    assert got["w"].shape == shapes["w"] and all(n_keep <= c <= n_keep + 8 for c in stats["kept"]["w"].values())
    assert stats["rows"] == D and all(lh[0] < lh[1] for lh in stats["thresholds"]["w"].values())
