"""
GPU tests of the dictionary level of task reconstruction (merge.reconstruct_task_vectors,
storage.reconstruct_tasks_from_artifacts, scripts/reconstruct_tasks.py): every task's own task vector -- or model, given
a base -- back out of the artifacts of a fused run or of adopted stored artifacts, all tasks of a plan in one
svdq_task_reconstruct.  The truth in every case is the per-parameter route on that task alone,

    merge_parameter(name, {t: comp[name][t]}, bases[name], {t: 1.0}, quantizer, shape, mask=..., include_noise=...,
                    noise_shrink=..., device="cuda")            (base + that, when a base is given)

and the comparison is bit for bit.  Shapes: tests/test_hip_adopt.py's ragged set and its two masked sizes.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [1, 3, 13, 255, 256, 257, 4095, 4096, 4097, 8193, 70001]
LACKING = ("p00257", "p04097")      # the "missing" configuration: task t03 lacks these two


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
    """One fused run per configuration ("full" / "missing"), its artifacts written once, and the truth of every
    (parameter, task) by the per-parameter route; shared by the tests and left unchanged."""
    if key in _RUNS:
        return _RUNS[key]
    from oracle import svd_hybrid_oracle as orc
    n = 8
    tasks = _tasks(n)
    tv = {t: {} for t in tasks}
    for rows in ROWS:
        for t, d in zip(tasks, orc.synthetic_deltas(rows, n, 31 * n + rows, rank=3)):
            tv[t][f"p{rows:05d}"] = d.cuda()
    if key == "missing":
        for name in LACKING:
            del tv[tasks[3]][name]
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    shapes = {f"p{rows:05d}": torch.Size([rows]) for rows in ROWS}
    d = str(tmp_path_factory.mktemp(key) / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n_: {"original_shape": list(s)} for n_, s in shapes.items()}},
                          cfg, d)
    g = torch.Generator().manual_seed(3)
    base = {name: torch.randn(s, generator=g).cuda() for name, s in shapes.items()}
    # the truth from the artifacts as LOADED (plain dictionaries: nothing batched about them)
    art = sq.load_all_artifacts(d, device="cpu")
    truth = _truth(sq, art["compressed"], art["bases"], {}, shapes, cfg)
    _RUNS[key] = (cfg, bases, comp, shapes, d, tasks, base, truth)
    return _RUNS[key]


def _truth(sq, comp, bases, masks, shapes, cfg):
    q = sq.RTVQQuantizer(num_bits=cfg.svd_low_bits, num_stages=cfg.svd_rtvq_stages)
    return {name: {t: sq.merge_parameter(name, {t: comp[name][t]}, bases[name], {t: 1.0}, q, shapes[name],
                                         mask=masks.get(name), include_noise=cfg.svd_include_noise,
                                         noise_shrink=cfg.svd_noise_shrink, device="cuda")
                   for t in comp[name]} for name in comp}


def _assert_equal(got, truth, tasks, base=None):
    """got {task: {param: tensor}} against truth {param: {task: tensor}} restricted to ``tasks``: same keys, same bits."""
    assert list(got) == list(tasks)
    for t in tasks:
        want_names = sorted(n for n in truth if t in truth[n])
        assert sorted(got[t]) == want_names, t
        for n in want_names:
            want = truth[n][t] if base is None else base[n] + truth[n][t]
            assert got[t][n].is_cuda and got[t][n].shape == want.shape and _bits(got[t][n], want), (t, n)


class _Spy:
    """Counters on the library's own entry points."""
    NAMES = ("svdq_task_reconstruct", "svdq_reconstruct", "svdq_rtvq_dequantize", "svdq_merge")

    def __init__(self, lib):
        self.lib, self.calls = lib, dict.fromkeys(self.NAMES, 0)

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(self.lib, n, self._wrap(n))
        return self.calls

    def _wrap(self, n):
        def call(*a):
            self.calls[n] += 1
            return self.real[n](*a)
        return call

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.lib, n, self.real[n])


def _counts(task_reconstruct, **other):
    return dict({"svdq_task_reconstruct": task_reconstruct, "svdq_reconstruct": 0, "svdq_rtvq_dequantize": 0,
                 "svdq_merge": 0}, **other)


# ------------------------------------------------------------------------------------------ fused and adopted
@pytest.mark.parametrize("key", ["full", "missing"])
@pytest.mark.parametrize("source", ["fused", "adopted"])
def test_every_task_of_a_run_and_of_its_stored_artifacts(sq, key, source, tmp_path_factory):
    cfg, bases, comp, shapes, d, tasks, base, truth = _run(sq, key, tmp_path_factory)
    if source == "adopted":
        art = sq.load_all_artifacts(d, device="cpu")
        bases, comp = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    plans = 2 if key == "missing" else 1
    with _Spy(sq._native.lib()) as calls:
        got = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
        with_base = sq.reconstruct_task_vectors(comp, bases, None, shapes, cfg, tasks=None, device="cuda",
                                                base_state_dict=base)
    assert calls == _counts(2 * plans), calls
    _assert_equal(got, truth, tasks)
    _assert_equal(with_base, truth, tasks, base)
    if key == "missing":
        for name in LACKING:
            assert name not in got[tasks[3]] and name in got[tasks[2]]
    # device="cpu" (the reference's default): the same values, on the CPU
    one = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[tasks[1]])
    assert all(not v.is_cuda and _bits(v.cuda(), truth[n][tasks[1]]) for n, v in one[tasks[1]].items())


def test_subset_of_tasks_and_freshness(sq, tmp_path_factory):
    cfg, bases, comp, shapes, d, tasks, base, truth = _run(sq, "missing", tmp_path_factory)
    pick = [tasks[6], tasks[3], tasks[0]]
    first = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=pick, device="cuda")
    _assert_equal(first, truth, pick)
    held = {t: {n: v.clone() for n, v in first[t].items()} for t in pick}
    # a second call with other tasks does not change what the first returned
    second = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[tasks[5], tasks[6]], device="cuda",
                                         base_state_dict=base)
    _assert_equal(second, truth, [tasks[5], tasks[6]], base)
    torch.cuda.synchronize()
    for t in pick:
        for n, v in first[t].items():
            assert _bits(v, held[t][n]), (t, n)
    with pytest.raises(ValueError, match="nobody"):
        sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[tasks[0], "nobody"], device="cuda")


def test_masked_parameters_with_noise_regions(sq, tmp_path):
    """Masks of density 0.6, svd_include_noise: the signal plan and the noise plan (scale = svd_noise_shrink) are each
    reconstructed in compacted rows and scattered per (parameter, task); base goes on afterwards.  On the fused run's
    dictionaries and on the adopted ones."""
    from oracle import svd_hybrid_oracle as orc
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
    base = {n: torch.randn(r, generator=g).cuda() for n, r in sizes.items()}
    d = str(tmp_path / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()}}, cfg, d)
    art = sq.load_all_artifacts(d, device="cpu")
    truth = _truth(sq, art["compressed"], art["bases"], masks, shapes, cfg)
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    for b, c in ((bases, comp), (ab, ac)):
        with _Spy(sq._native.lib()) as calls:
            got = sq.reconstruct_task_vectors(c, b, masks, shapes, cfg, device="cuda", base_state_dict=base)
        plans = {id(b[n][r]._batch[0].plan) for n in sizes for r in ("masked", "noise")}
        assert calls == _counts(len(plans)), calls      # one call per plan, whether the regions share one or not
        _assert_equal(got, truth, tasks, base)
    # the noise region matters: the rows outside the mask are not zero
    outside = truth["m70001"][tasks[0]][~masks["m70001"]]
    assert float(outside.abs().max()) > 0


def test_an_edited_entry_goes_per_parameter_with_the_same_bits(sq, tmp_path_factory):
    cfg, _, _, shapes, d, tasks, base, truth = _run(sq, "full", tmp_path_factory)
    from svdq_amd import merge as mg
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    name = "p04097"
    ac[name][tasks[2]] = dict(ac[name][tasks[2]])      # an equal copy: the entry no longer is what adoption handed out
    assert mg._batched_entry(name, ac, ab) is None and mg._batched_entry("p08193", ac, ab) is not None
    with _Spy(sq._native.lib()) as calls:
        got = sq.reconstruct_task_vectors(ac, ab, {}, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls["svdq_task_reconstruct"] == 1 and calls["svdq_merge"] == 0, calls
    assert calls["svdq_reconstruct"] == len(tasks), calls      # that parameter alone, task by task
    _assert_equal(got, truth, tasks, base)


# ------------------------------------------------------------------------------------------ stored artifacts, script
def test_script_writes_every_task_model(sq, tmp_path):
    """scripts/reconstruct_tasks.py as a user would call it, on the three-parameter, six-task set of
    test_reconstruct_from_artifacts_takes_the_batched_route; one base key the artifacts do not cover."""
    from oracle import svd_hybrid_oracle as orc
    tasks = ["A", "B", "C", "D", "E", "F"]
    shapes = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (32, 64)}
    tv = {t: {} for t in tasks}
    for pi, (n, shp) in enumerate(sorted(shapes.items())):
        for t, x in zip(tasks, orc.synthetic_deltas(int(np.prod(shp)), len(tasks), 500 + pi)):
            tv[t][n] = x.view(shp).cuda()
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    d = str(tmp_path / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()}},
                          cfg, d)
    base = {n: torch.randn(s) for n, s in shapes.items()}
    base["head.bias"] = torch.randn(10)
    torch.save(base, str(tmp_path / "base.pt"))
    tshapes = {n: torch.Size(s) for n, s in shapes.items()}
    truth = _truth(sq, comp, bases, {}, tshapes, cfg)
    # in process: one svdq_task_reconstruct for the plan, nothing per parameter or per task
    with _Spy(sq._native.lib()) as calls:
        models = sq.reconstruct_tasks_from_artifacts(d, base, tasks=["C", "A"], device="cuda")
    assert calls == _counts(1), calls
    assert list(models) == ["C", "A"]
    for t in models:
        assert sorted(models[t]) == sorted(base)
        for n in shapes:
            assert _bits(models[t][n], base[n].cuda() + truth[n][t]), (t, n)
        assert _bits(models[t]["head.bias"], base["head.bias"])
    with pytest.raises(ValueError, match="Z"):
        sq.reconstruct_tasks_from_artifacts(d, base, tasks=["A", "Z"], device="cuda")
    # the script
    out = str(tmp_path / "models")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reconstruct_tasks.py"), "--artifact-dir", d,
                         "--base-model-path", str(tmp_path / "base.pt"), "--output-dir", out, "--device", "cuda"],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert sorted(os.listdir(out)) == [f"{t}.pt" for t in tasks]
    for t in tasks:
        sd = torch.load(os.path.join(out, f"{t}.pt"), weights_only=True)
        assert sorted(sd) == sorted(base)
        for n in shapes:
            assert _bits(sd[n].cuda(), base[n].cuda() + truth[n][t]), (t, n)
        assert _bits(sd["head.bias"], base["head.bias"])
