"""
TALL masks and the consensus merge from a saved store (storage.consensus_merge_from_artifacts,
scripts/consensus_merge.py): the same bits as the dictionary route on the fused run that wrote the store, the store's
files untouched; the written TALL_mask_{T}task.npz read back by the package's own loaders (load_tall_mask_file,
combine_tall_masks_packed -- the compressor's mask path) gives the model's masks; and no task model is reconstructed on
the way.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tall_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (130, 64), "head.w": (257, 33)}
TASKS = ["A", "B", "C", "D", "E", "F"]
TALL = ("svdq_plan_tall_consensus",)
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
    """A fused run of six tasks over four parameters (task F lacks one), its store on disk, a base checkpoint with keys
    the store does not cover (one sorts first, one between, one last) and the model's masks per parameter."""
    from oracle import svd_hybrid_oracle as orc
    tmp = tmp_path_factory.mktemp("tall_store")
    tv = {t: {} for t in TASKS}
    for pi, (n, shp) in enumerate(sorted(SHAPES.items())):
        for t, x in zip(TASKS, orc.synthetic_deltas(int(np.prod(shp)), len(TASKS), 900 + pi)):
            tv[t][n] = x.view(shp).cuda()
    del tv["F"]["enc/w2"]
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_energy_threshold=0.9, svd_max_rank=1, svd_low_bits=4, svd_rtvq_stages=1)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    d = str(tmp / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()}},
                          cfg, d)
    g = torch.Generator().manual_seed(4)
    base = {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}
    base["a.embed"] = torch.randn(5, 3, generator=g)
    base["enc.ln"] = torch.randn(7, generator=g)
    base["head.z"] = torch.randn(10, generator=g)
    torch.save(base, str(tmp / "base.pt"))
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    assert all(bool(torch.isfinite(x).all()) for per in recon.values() for x in per.values())
    names = sorted(SHAPES)
    sizes = {n: int(np.prod(SHAPES[n])) for n in names}
    v, has = tm.stack_values(recon, TASKS, names, sizes)
    return cfg, bases, comp, shapes, d, base, str(tmp), (names, sizes, v, has)


def test_store_and_script_equal_the_dictionary_route_and_the_mask_file_round_trips(sq, store):
    cfg, bases, comp, shapes, d, base, tmp, (names, sizes, v, has) = store
    T = len(TASKS)
    kw = dict(tall_lambda=0.4, k=2, scaling=0.7)
    dev_base = {n: b.cuda() for n, b in base.items() if n in shapes}
    want, wmasks, wstats = sq.consensus_merge_parameters(comp, bases, shapes, cfg, base_state_dict=dev_base,
                                                         reference_state_dict=base, return_masks=True, device="cuda",
                                                         return_stats=True, **kw)
    before = _digest(d)
    out_path = os.path.join(tmp, "merged_api.pt")
    mask_dir = os.path.join(tmp, "masks")
    os.makedirs(mask_dir)
    mask_path = os.path.join(mask_dir, f"TALL_mask_{T}task.npz")
    with _Spy(sq._native.lib(), TALL + NEVER) as calls:
        res = sq.consensus_merge_from_artifacts(d, os.path.join(tmp, "base.pt"), out_path, mask_path, device="cuda", **kw)
    # task F lacks a parameter: adoption makes two plans, one launch each
    assert calls == {"svdq_plan_tall_consensus": 2, "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}, calls
    assert _digest(d) == before
    merged = res["merged_state_dict"]
    assert sorted(merged) == sorted(base)
    for n in shapes:
        assert merged[n].shape == shapes[n] and merged[n].dtype is torch.float32 and _bits(merged[n], want[n]), n
    for n in ("a.embed", "enc.ln", "head.z"):
        assert _bits(merged[n], base[n])
    rows = sum(sizes.values())
    assert res["stats"] == wstats and res["stats"]["rows"] == rows and sum(res["stats"]["agreement"]) == rows
    assert sorted(res["stats"]["active"]) == TASKS
    saved = torch.load(out_path, weights_only=True)
    assert sorted(saved) == sorted(base) and all(_bits(saved[n], merged[n]) for n in saved)
    # ---- the model: merged values, statistics, and the masks per parameter
    base_flat = tm.stack_values({"b": base}, ["b"], names, sizes)[0][0]
    mwant, wm, ws = tm.consensus_merge(v, has, 0.4, 2, 0.7, base_flat)
    for n, x in tm.split_rows(mwant, names, sizes).items():
        assert np.array_equal(merged[n].cpu().numpy().reshape(-1).view(np.uint32), x.view(np.uint32)), n
    assert [res["stats"]["active"][t] for t in TASKS] == ws["active"].tolist()
    assert res["stats"]["agreement"] == ws["agreement"].tolist()
    density = wm.sum(axis=1) / has.sum(axis=1)
    assert (density > 0.05).all() and (density < 0.95).all(), density      # the model's masks are neither empty nor full
    per_param = tm.split_rows(wm, names, sizes)
    assert os.listdir(mask_dir) == [f"TALL_mask_{T}task.npz"]      # the caller's name, no suffix appended
    z = np.load(mask_path, allow_pickle=False)
    total = sum(b.numel() for b in base.values())
    assert sorted(z.files) == TASKS
    for t in TASKS:
        assert z[t].dtype == np.uint8 and z[t].shape == ((total + 7) // 8,)
        assert np.array_equal(z[t], wmasks[t].cpu().numpy()) and np.array_equal(z[t], res["masks"][t].cpu().numpy())
    # ---- read back by load_tall_mask_file with the base as the reference
    loaded = sq.load_tall_mask_file(mask_path, base)
    assert sorted(loaded) == TASKS
    for g, t in enumerate(TASKS):
        assert sorted(loaded[t]) == sorted(base)
        for n in names:
            assert loaded[t][n].dtype is torch.bool and loaded[t][n].shape == shapes[n]
            assert np.array_equal(loaded[t][n].numpy().reshape(-1), per_param[n][g]), (t, n)
        for n in ("a.embed", "enc.ln", "head.z"):
            assert not loaded[t][n].any()
    assert not loaded["F"]["enc/w2"].any() and loaded["E"]["enc/w2"].any()      # F lacks it
    assert sq.cli._find_tall_mask_file(mask_dir, T) == mask_path
    # ---- the same file through the compressor's mask path: the packed vote on the device
    union = sq.combine_tall_masks_packed(mask_path, TASKS, base, "union", device="cuda")
    for n in names:
        assert np.array_equal(union[n].cpu().numpy().reshape(-1), per_param[n].any(axis=0)), n
    for n in ("a.embed", "enc.ln", "head.z"):
        assert not union[n].any()
    # ---- the script: masks and merge over a subset of tasks
    sub = ["B", "D", "F"]
    want2, m2, wstats2 = sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=0.25, k=1, tasks=sub,
                                                       base_state_dict=dev_base, reference_state_dict=base,
                                                       return_masks=True, device="cuda", return_stats=True)
    script_out, script_masks = os.path.join(tmp, "merged_script.pt"), os.path.join(tmp, "TALL_mask_3task.npz")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "consensus_merge.py"), "--artifact-dir", d,
                         "--base-model-path", os.path.join(tmp, "base.pt"), "--output-path", script_out, "--mask-output",
                         script_masks, "--tall-lambda", "0.25", "--k", "1", "--tasks", "B", "F", "D"],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [json.loads(ln) for ln in rc.stdout.splitlines() if ln.startswith("{")]
    assert lines[0] == {"active": wstats2["active"]} and list(lines[0]["active"]) == sub
    assert lines[1] == {"agreement": wstats2["agreement"], "rows": rows} and len(lines[1]["agreement"]) == 4
    saved = torch.load(script_out, weights_only=True)
    assert sorted(saved) == sorted(base)
    for n in shapes:
        assert _bits(saved[n], want2[n]), n
    z2 = np.load(script_masks, allow_pickle=False)
    assert sorted(z2.files) == sub and all(np.array_equal(z2[t], m2[t].cpu().numpy()) for t in sub)
    assert _digest(d) == before
    with pytest.raises(ValueError, match="Z"):
        sq.consensus_merge_from_artifacts(d, base, tasks=["A", "Z"], device="cuda")
    with pytest.raises(ValueError, match=r"k must be an integer in \[0, 6\]"):
        sq.consensus_merge_from_artifacts(d, base, k=7, device="cuda")


def test_a_masked_store_is_refused_by_name(sq, tmp_path):
    from oracle import svd_hybrid_oracle as orc
    tasks = TASKS[:4]
    g = torch.Generator().manual_seed(9)
    tv = {t: {"m.w": x.cuda()} for t, x in zip(tasks, orc.synthetic_deltas(4097, 4, 5))}
    masks = {"m.w": (torch.rand(4097, generator=g) < 0.6).cuda()}
    mcfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2,
                              svd_min_mask_size=10)
    mb, mc = sq.run_basis_and_compress(tv, masks, mcfg, "cuda")
    with pytest.raises(ValueError, match=r"consensus_merge_parameters: parameter 'm\.w'.*masked run.*the consensus merge"):
        sq.consensus_merge_parameters(mc, mb, {"m.w": torch.Size([4097])}, mcfg, device="cuda")
    with pytest.raises(ValueError, match=r"tall_masks_from_store: parameter 'm\.w'.*masked run.*the TALL mask"):
        sq.tall_masks_from_store(mc, mb, {"m.w": torch.Size([4097])}, mcfg, device="cuda")
    md = str(tmp_path / "masked")
    sq.save_all_artifacts(mb, mc, {"per_parameter": {"m.w": {"original_shape": [4097]}}}, mcfg, md)
    with pytest.raises(ValueError, match=r"'m\.w'.*masked run"):
        sq.consensus_merge_from_artifacts(md, {"m.w": torch.zeros(4097)}, device="cuda")
