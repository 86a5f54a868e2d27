"""
The EMR merge from a saved store (storage.emr_from_artifacts, storage.emr_task_model_from_files, scripts/emr_merge.py):
the same bits as the dictionary route on the fused run that wrote the store, the store's files untouched; the written
EMR_mask_{T}task.npz read back by the package's own loader (load_tall_mask_file) gives the model's masks; the script's
two steps, each a fresh process, write the same files and the same task model; and no task model is reconstructed on
the way.

One numerical sanity check that is no gate on accuracy: the relative L2 error of the EMR task vector
lambda_t * (M_t (.) tau_uni) against v_t is printed per task and asserted only to be finite and below 1 (better than
predicting zero).  On these seeded inputs the model alone (tests/emr_model.py on the task deltas the store is made from,
on the CPU) gives 0.42 .. 0.73 with mask densities of 0.68 .. 0.86.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import emr_model as em
import tall_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (130, 64), "head.w": (257, 33)}
TASKS = ["A", "B", "C", "D", "E", "F"]
EMR = ("svdq_plan_emr_elect", "svdq_emr_apply")
NEVER = ("svdq_task_reconstruct", "svdq_reconstruct")
SHARED = 0.01      # the generator's own scale a


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
    the store does not cover, and the model of the values the store reconstructs."""
    from oracle import svd_hybrid_oracle as orc
    tmp = tmp_path_factory.mktemp("emr_store")
    tv = {t: {} for t in TASKS}
    for pi, (n, shp) in enumerate(sorted(SHAPES.items())):
        rows = int(np.prod(shp))
        # what every task moved alike, at the scale of what each moved on its own: without it the generator's tasks point
        # along and against each other in three directions, and one vector with one scalar per task serves the
        # outvoted ones worse than zero would (relative error up to 1.5 with the model on the CPU)
        shared = SHARED * torch.randn(rows, generator=torch.Generator().manual_seed(77 + pi))
        for t, x in zip(TASKS, orc.synthetic_deltas(rows, len(TASKS), 900 + pi)):
            tv[t][n] = (x + shared).view(shp).cuda()
    del tv["F"]["enc/w2"]
    cfg = sq.SVDHybridConfig(tasks=TASKS, svd_energy_threshold=0.9, svd_max_rank=1, svd_low_bits=4, svd_rtvq_stages=1)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    d = str(tmp / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()}},
                          cfg, d)
    g = torch.Generator().manual_seed(4)
    base = {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}
    base["a.embed"] = torch.randn(5, 3, generator=g)
    base["head.z"] = torch.randn(10, generator=g)
    torch.save(base, str(tmp / "base.pt"))
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    assert all(bool(torch.isfinite(x).all()) for per in recon.values() for x in per.values())
    names = sorted(SHAPES)
    sizes = {n: int(np.prod(SHAPES[n])) for n in names}
    v, has = tm.stack_values(recon, TASKS, names, sizes)
    return cfg, bases, comp, shapes, d, base, str(tmp), (names, sizes, v, has, em.emr_merge(v, has))


def test_store_route_and_script_equal_the_dictionary_route(sq, store):
    cfg, bases, comp, shapes, d, base, tmp, (names, sizes, v, has, model) = store
    T, rows = len(TASKS), sum(sizes.values())
    want_u, want_m, want_r, want_s = sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True)
    before = _digest(d)
    out_dir = os.path.join(tmp, "emr_api")
    with _Spy(sq._native.lib(), EMR + NEVER) as calls:
        res = sq.emr_from_artifacts(d, out_dir, device="cuda")
    # task F lacks a parameter: adoption makes two plans, one launch each
    assert calls == {"svdq_plan_emr_elect": 2, "svdq_emr_apply": 0, "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}
    assert _digest(d) == before
    assert sorted(os.listdir(out_dir)) == [f"EMR_mask_{T}task.npz", "emr_rescalers.json", "emr_unified.pt"]
    assert res["rescalers"] == want_r and res["stats"] == want_s and res["stats"]["rows"] == rows
    for n in names:
        assert res["unified"][n].shape == shapes[n] and _bits(res["unified"][n], want_u[n]), n
    for t in TASKS:
        assert torch.equal(res["masks"][t].cpu(), want_m[t].cpu()), t
    # ---- the model: tau_uni, the masks per parameter through the package's loader, the sums
    for n, x in tm.split_rows(model["tau"], names, sizes).items():
        assert np.array_equal(res["unified"][n].cpu().numpy().reshape(-1).view(np.uint32), x.view(np.uint32)), n
    unified_file = torch.load(os.path.join(out_dir, "emr_unified.pt"), weights_only=True)
    assert sorted(unified_file) == names and all(_bits(unified_file[n], want_u[n]) for n in names)
    loaded = sq.load_tall_mask_file(res["paths"]["masks"], unified_file)
    per_param = tm.split_rows(model["masks"], names, sizes)
    assert sorted(loaded) == TASKS
    for g, t in enumerate(TASKS):
        for n in names:
            assert loaded[t][n].dtype is torch.bool and loaded[t][n].shape == shapes[n]
            assert np.array_equal(loaded[t][n].numpy().reshape(-1), per_param[n][g]), (t, n)
        n_rows = int(has[g].sum())
        assert abs(res["stats"]["abs_sum"][t] - model["A"][g]) <= n_rows * 2.0 ** -52 * model["A"][g], t
        assert abs(res["stats"]["masked_sum"][t] - model["B"][g]) <= n_rows * 2.0 ** -52 * model["B"][g], t
        assert res["stats"]["active"][t] == int(model["masks"][g].sum())
    assert not loaded["F"]["enc/w2"].any() and loaded["E"]["enc/w2"].any()      # F lacks it
    density = model["masks"].sum(axis=1) / has.sum(axis=1)
    assert (density > 0.05).all() and (density < 0.95).all(), density      # neither empty nor full
    record = json.load(open(os.path.join(out_dir, "emr_rescalers.json")))
    assert record["rescalers"] == want_r and record["tasks"] == TASKS and record["rows"] == rows
    # ---- a task's model from the files: one launch, the bits of the in-memory route, the base's other tensors cloned
    dev_base = {n: b.cuda() for n, b in base.items() if n in shapes}
    for t in ("C", "F"):
        want = sq.emr_task_state_dict(want_u, want_m, want_r, t, base_state_dict=dev_base, device="cuda")
        path = os.path.join(tmp, f"task_{t}.pt")
        with _Spy(sq._native.lib(), EMR + NEVER) as calls:
            got = sq.emr_task_model_from_files(out_dir, t, os.path.join(tmp, "base.pt"), path, device="cuda")
        assert calls == {"svdq_plan_emr_elect": 0, "svdq_emr_apply": 1, "svdq_task_reconstruct": 0, "svdq_reconstruct": 0}
        assert got["rescaler"] == want_r[t] and sorted(got["state_dict"]) == sorted(base)
        saved = torch.load(path, weights_only=True)
        g = TASKS.index(t)
        base_flat = tm.stack_values({"b": base}, ["b"], names, sizes)[0][0]
        mwant = tm.split_rows(em.task_model(model["tau"], model["masks"][g], want_r[t], base_flat), names, sizes)
        for n in names:
            assert got["state_dict"][n].shape == shapes[n] and _bits(got["state_dict"][n], want[n]), (t, n)
            assert _bits(saved[n], want[n]), (t, n)
            assert np.array_equal(saved[n].numpy().reshape(-1).view(np.uint32), mwant[n].view(np.uint32)), (t, n)
        for n in ("a.embed", "head.z"):
            assert _bits(got["state_dict"][n], base[n]) and _bits(saved[n], base[n])
    # ---- the sanity check that is no gate: the EMR task vector against the task's own, per task
    for g, t in enumerate(TASKS):
        approx = em.task_model(model["tau"], model["masks"][g], want_r[t]).astype(np.float64)
        own = np.where(has[g], v[g], 0).astype(np.float64)
        rel = float(np.linalg.norm(approx - own) / np.linalg.norm(own))
        print(f"task {t}: rescaler {want_r[t]:.4f}, relative L2 error of the EMR task vector {rel:.4f}")
        assert np.isfinite(rel) and rel < 1.0, (t, rel)
    # ---- the script's two steps, each a fresh process, over a subset of tasks
    sub = ["B", "D", "F"]
    u2, m2, r2, s2 = sq.emr_merge_parameters(comp, bases, shapes, cfg, tasks=sub, device="cuda", return_stats=True)
    script = os.path.join(ROOT, "scripts", "emr_merge.py")
    script_dir = os.path.join(tmp, "emr_script")
    rc = subprocess.run([sys.executable, script, "--artifact-dir", d, "--output-dir", script_dir, "--tasks", "B", "F", "D"],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    lines = [json.loads(ln) for ln in rc.stdout.splitlines() if ln.startswith("{")]
    assert lines[0] == {"rescalers": r2} and list(lines[0]["rescalers"]) == sub
    assert lines[1] == {"active": s2["active"], "rows": rows}
    assert sorted(os.listdir(script_dir)) == ["EMR_mask_3task.npz", "emr_rescalers.json", "emr_unified.pt"]
    z = np.load(os.path.join(script_dir, "EMR_mask_3task.npz"), allow_pickle=False)
    assert sorted(z.files) == sub and all(np.array_equal(z[t], m2[t].cpu().numpy()) for t in sub)
    model_path = os.path.join(tmp, "task_D_script.pt")
    rc = subprocess.run([sys.executable, script, "--output-dir", script_dir, "--task", "D", "--base-model-path",
                         os.path.join(tmp, "base.pt"), "--output-path", model_path],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert json.loads(rc.stdout.splitlines()[0]) == {"task": "D", "rescaler": r2["D"]}
    want = sq.emr_task_state_dict(u2, m2, r2, "D", base_state_dict=dev_base, device="cuda")
    saved = torch.load(model_path, weights_only=True)
    assert sorted(saved) == sorted(base)
    for n in names:
        assert _bits(saved[n], want[n]), n
    assert _digest(d) == before
    with pytest.raises(ValueError, match="Z"):
        sq.emr_from_artifacts(d, os.path.join(tmp, "nowhere"), tasks=["A", "Z"], device="cuda")
    assert not os.path.exists(os.path.join(tmp, "nowhere"))
    with pytest.raises(ValueError, match="unknown task 'A'"):
        sq.emr_task_model_from_files(script_dir, "A", base, device="cuda")


def test_a_masked_store_is_refused_by_name(sq, tmp_path):
    from oracle import svd_hybrid_oracle as orc
    tasks = TASKS[:4]
    g = torch.Generator().manual_seed(9)
    tv = {t: {"m.w": x.cuda()} for t, x in zip(tasks, orc.synthetic_deltas(4097, 4, 5))}
    masks = {"m.w": (torch.rand(4097, generator=g) < 0.6).cuda()}
    mcfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=2, svd_low_bits=4, svd_rtvq_stages=2,
                              svd_min_mask_size=10)
    mb, mc = sq.run_basis_and_compress(tv, masks, mcfg, "cuda")
    with pytest.raises(ValueError, match=r"emr_merge_parameters: parameter 'm\.w'.*masked run.*the EMR merge"):
        sq.emr_merge_parameters(mc, mb, {"m.w": torch.Size([4097])}, mcfg, device="cuda")
    md = str(tmp_path / "masked")
    sq.save_all_artifacts(mb, mc, {"per_parameter": {"m.w": {"original_shape": [4097]}}}, mcfg, md)
    with pytest.raises(ValueError, match=r"'m\.w'.*masked run"):
        sq.emr_from_artifacts(md, str(tmp_path / "out"), device="cuda")
