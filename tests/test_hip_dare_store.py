"""
The DARE merge from a saved store (storage.dare_merge_from_artifacts, scripts/dare_merge.py): the same bits as the
dictionary route on the fused run that wrote the store, the store's files untouched; the refusals (a masked run's store, a
parameter adoption declined) name the parameter under this merge's name; the footprint stays under two models where the
materialised route holds eight; and no task model is reconstructed on the way.
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
DARE = ("svdq_plan_dare_merge",)
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
    tmp = tmp_path_factory.mktemp("dare_store")
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
    kw = dict(drop_rate=0.7, seed=(5 << 32) + 11, scaling=0.7, weights={t: 0.5 + 0.25 * i for i, t in enumerate(TASKS)})
    dev_base = {n: b.cuda() for n, b in base.items() if n in shapes}
    want, wstats = sq.dare_merge_parameters(comp, bases, shapes, cfg, base_state_dict=dev_base, device="cuda",
                                            return_stats=True, **kw)
    before = _digest(d)
    out_path = os.path.join(tmp, "merged_api.pt")
    with _Spy(sq._native.lib(), DARE + NEVER) as calls:
        res = sq.dare_merge_from_artifacts(d, os.path.join(tmp, "base.pt"), out_path, device="cuda", **kw)
    # task F lacks a parameter: adoption makes two plans, one launch each
    assert calls == {"svdq_plan_dare_merge": 2, "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}, calls
    assert _digest(d) == before
    merged = res["merged_state_dict"]
    assert sorted(merged) == sorted(base)
    for n in shapes:
        assert merged[n].shape == shapes[n] and merged[n].dtype is torch.float32 and _bits(merged[n], want[n]), n
    assert _bits(merged["head.bias"], base["head.bias"])
    rows = sum(int(np.prod(s)) for s in SHAPES.values())
    assert res["stats"] == wstats and res["stats"]["rows"] == rows
    assert sorted(res["stats"]["kept"]) == TASKS and res["stats"]["drop_threshold"] == int(0.7 * 2.0 ** 32)
    assert all(0 < c < rows for c in res["stats"]["kept"].values())
    saved = torch.load(out_path, weights_only=True)
    assert sorted(saved) == sorted(base) and all(_bits(saved[n], merged[n]) for n in saved)
    # ---- the script: task arithmetic (--drop-rate 0) over a subset of tasks with weights
    want2, wstats2 = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.0, tasks=["B", "F", "D"],
                                              weights={"B": 0.5, "D": 2.0, "F": 1.5}, base_state_dict=dev_base,
                                              device="cuda", return_stats=True)
    script_out = os.path.join(tmp, "merged_script.pt")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "dare_merge.py"), "--artifact-dir", d,
                         "--base-model-path", os.path.join(tmp, "base.pt"), "--output-path", script_out, "--drop-rate",
                         "0", "--tasks", "B", "F", "D", "--weights", "0.5", "2.0", "1.5"],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [json.loads(ln) for ln in rc.stdout.splitlines() if ln.startswith("{")]
    assert lines[0] == {"kept": wstats2["kept"]} and list(lines[0]["kept"]) == ["B", "D", "F"]
    assert lines[1] == {"rows": rows, "drop_threshold": 0}
    enc_w2 = int(np.prod(SHAPES["enc/w2"]))
    assert wstats2["kept"] == {"B": rows, "D": rows, "F": rows - enc_w2}      # nothing dropped; F lacks enc/w2
    saved = torch.load(script_out, weights_only=True)
    assert sorted(saved) == sorted(base)
    for n in shapes:
        assert _bits(saved[n], want2[n]), n
    assert _digest(d) == before
    with pytest.raises(ValueError, match="Z"):
        sq.dare_merge_from_artifacts(d, base, tasks=["A", "Z"], device="cuda")


def test_two_calls_give_identical_bits(sq, store):
    cfg, bases, comp, shapes, d, base, tmp = store
    one, s1 = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.9, seed=3, device="cuda", return_stats=True)
    two, s2 = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.9, seed=3, device="cuda", return_stats=True)
    assert s1 == s2 and all(_bits(one[n], two[n]) and one[n].data_ptr() != two[n].data_ptr() for n in shapes)


def test_a_masked_store_and_a_declined_parameter_are_refused_by_name(sq, store, tmp_path):
    from oracle import svd_hybrid_oracle as orc
    cfg, bases, comp, shapes, d, base, tmp = store
    # ---- a parameter adoption declines (a basis dtype no plan holds) stays a plain dictionary
    art = sq.load_all_artifacts(d, device="cpu")
    art["bases"]["enc.b1"]["masked"]["U_high"] = art["bases"]["enc.b1"]["masked"]["U_high"].double()
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    with pytest.raises(ValueError, match=r"dare_merge_parameters: parameter 'enc\.b1' is not backed by a plan"):
        sq.dare_merge_parameters(ac, ab, shapes, cfg, device="cuda")
    # ---- a masked run's store holds the selected rows only
    tasks = TASKS[:4]
    g = torch.Generator().manual_seed(9)
    tv = {t: {"m.w": x.cuda()} for t, x in zip(tasks, orc.synthetic_deltas(4097, 4, 5))}
    masks = {"m.w": (torch.rand(4097, generator=g) < 0.6).cuda()}
    mcfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2,
                              svd_min_mask_size=10)
    mb, mc = sq.run_basis_and_compress(tv, masks, mcfg, "cuda")
    with pytest.raises(ValueError, match=r"dare_merge_parameters: parameter 'm\.w'.*masked run.*the DARE merge"):
        sq.dare_merge_parameters(mc, mb, {"m.w": torch.Size([4097])}, mcfg, device="cuda")
    md = str(tmp_path / "masked")
    sq.save_all_artifacts(mb, mc, {"per_parameter": {"m.w": {"original_shape": [4097]}}}, mcfg, md)
    with pytest.raises(ValueError, match=r"'m\.w'.*masked run"):
        sq.dare_merge_from_artifacts(md, {"m.w": torch.zeros(4097)}, device="cuda")


def test_footprint_stays_under_two_models_and_no_task_model_is_formed(sq):
    """One parameter of 2^22 rows, 8 tasks: the rise of the peak during the merge is the output plus small tables --
    under 2 x 4 D bytes (the bound of tests/test_hip_ties_store.py), where reconstruct_task_vectors for all tasks holds
    8 x 4 D."""
    D, T = 1 << 22, 8
    tasks = [f"t{i}" for i in range(T)]
    g = torch.Generator(device="cuda").manual_seed(2)
    B = torch.randn(D, 3, generator=g, device="cuda")
    tv = {t: {"w": 0.01 * (B @ torch.randn(3, generator=g, device="cuda")) + 0.002 * torch.randn(D, generator=g, device="cuda")}
          for t in tasks}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    del tv, B
    shapes = {"w": torch.Size([D])}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with _Spy(sq._native.lib(), DARE + NEVER) as calls:
        got, stats = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.9, seed=1, device="cuda",
                                              return_stats=True)
        torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes = {rise / (4 * D):.3f} models of {4 * D} bytes")
    assert rise < 2 * 4 * D, rise
    assert calls == {"svdq_plan_dare_merge": 1, "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}, calls
    # the kept counts at 2^22 rows: within six binomial standard deviations of D (1 - p)
    sd = (D * 0.9 * 0.1) ** 0.5
    assert got["w"].shape == shapes["w"] and stats["rows"] == D
    assert all(abs(c - D * 0.1) <= 6 * sd for c in stats["kept"].values()), stats["kept"]
