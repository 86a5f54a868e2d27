"""
GPU tests of the dictionary level of the store Gram: clustering.task_gram_from_artifacts /
cluster_tasks_from_artifacts, storage.remerge_from_artifacts, scripts/remerge.py and scripts/add_task.py --weighting
cluster.

Two planted groups of four tasks over three parameters of 4096 elements: every task is 5 x its group's direction plus
an individual part.  The truth of a Gram is numpy fp64 on the STORED artifacts (Delta = U C + mean per parameter and
region, c_low through the C model of the quantizer) and the bound is tests/test_hip_store_gram.py's, summed over the
entries: (256 + r + 3) 2^-24 |C'|^T (|A|^T |A|) |C'|.  The per-parameter route reconstructs in fp32 (an fma chain of
r + 2 terms per element) before its fp64 Gram: 2 (r + 3) 2^-24 of the same magnitude, inside the same bound.
"""

import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24
SHAPES = {"blk.a": (64, 64), "blk.b": (4096,), "blk.c": (32, 128)}
GROUP_A = [f"a{i}" for i in range(4)]
GROUP_B = [f"b{i}" for i in range(4)]
TASKS = GROUP_A + GROUP_B
NEW = "a_new"
MASKED = "blk.a"
LACKING = ("b3", ("blk.b", "blk.c"))      # one task lacks two parameters


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle as o
    o.build_c_oracle()
    return o


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().contiguous().view(torch.int32),
                                                                    b.cpu().contiguous().view(torch.int32))


def _world(sq, tmp, *, ragged, masked):
    """Base model, checkpoints (the eight tasks and a ninth in group A), task vectors, the fused run and its store."""
    g = torch.Generator().manual_seed(77)
    s = 0.01
    base, ckpt = {}, {t: {} for t in TASKS + [NEW]}
    for name, shape in SHAPES.items():
        base[name] = torch.randn(shape, generator=g)
        dirs = {"a": torch.randn(shape, generator=g), "b": torch.randn(shape, generator=g)}
        for t in TASKS + [NEW]:
            ckpt[t][name] = base[name] + 5.0 * s * dirs[t[0]] + s * torch.randn(shape, generator=g)
    base["head.bias"] = torch.randn(7, generator=g)          # a tensor the store does not cover
    for t in ckpt:
        ckpt[t]["head.bias"] = base["head.bias"].clone()
    tv = {t: {n: (ckpt[t][n] - base[n]).cuda() for n in SHAPES} for t in TASKS}
    if ragged:
        for n in LACKING[1]:
            del tv[LACKING[0]][n]
    masks = {MASKED: (torch.rand(SHAPES[MASKED], generator=g) < 0.6).cuda()} if masked else {}
    cfg = sq.SVDHybridConfig(tasks=list(TASKS), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_include_noise=masked, svd_noise_shrink=0.5, svd_min_mask_size=10,
                             svd_cluster_k=2)
    bases, comp = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    d = str(tmp / "art")
    diag = {"per_parameter": {n: {"original_shape": list(sh)} for n, sh in SHAPES.items()},
            "task_weights": {t: (1.0 + 0.1 * i) / sum(1.0 + 0.1 * j for j in range(len(TASKS)))
                             for i, t in enumerate(TASKS)}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    base_path = str(tmp / "base.pt")
    torch.save(base, base_path)
    return dict(dir=d, base=base, base_path=base_path, ckpt=ckpt, tv=tv, masks=masks, cfg=cfg, bases=bases, comp=comp,
                tmp=tmp)


@pytest.fixture(scope="module")
def ragged(sq, tmp_path_factory):
    """b3 lacks two parameters; blk.a is masked (density 0.6) with a noise region."""
    return _world(sq, tmp_path_factory.mktemp("ragged"), ragged=True, masked=True)


@pytest.fixture(scope="module")
def plain(sq, tmp_path_factory):
    return _world(sq, tmp_path_factory.mktemp("plain"), ragged=False, masked=False)


def _stored_truth(art, orc):
    """(G64, bound, tasks) from loaded (un-adopted) dictionaries."""
    bases, comp = art["bases"], art["compressed"]
    tasks = sorted({t for per in comp.values() for t in per})
    pos = {t: i for i, t in enumerate(tasks)}
    G = np.zeros((len(tasks), len(tasks)))
    bound = np.zeros_like(G)
    for name in sorted(comp):
        for region, key in (("masked", "masked"), ("noise", "unmasked")):
            rb = bases[name].get(region)
            if rb is None:
                continue
            present = sorted(t for t, a in comp[name].items() if a.get(key) is not None)
            if not present:
                continue
            A = torch.cat([rb["U_high"].double(), rb["U_low"].double()], dim=1).numpy()
            r = A.shape[1]
            cols = []
            for t in present:
                a = comp[name][t][key]
                pay = a["c_low_quant"]["payloads"]
                low = np.zeros(0)
                if pay:
                    low = orc.rtvq_dequantize({"codes": np.stack([p["quantized"].numpy().reshape(-1) for p in pay]),
                                               "scale": np.array([float(p["scale"]) for p in pay], np.float32),
                                               "zero_point": np.array([float(p["zero_point"]) for p in pay], np.float32)})
                cols.append(np.concatenate([a["c_high_fp16"].double().numpy().reshape(-1), low.reshape(-1).astype(np.float64)]))
            C = np.stack(cols, axis=1)
            if rb.get("mean") is not None:
                A = np.concatenate([A, rb["mean"].double().numpy().reshape(-1, 1)], axis=1)
                C = np.concatenate([C, np.ones((1, len(present)))], axis=0)
            assert np.isfinite(A).all() and np.isfinite(C).all()
            delta = A @ C
            idx = np.array([pos[t] for t in present])
            G[np.ix_(idx, idx)] += delta.T @ delta
            bound[np.ix_(idx, idx)] += (256 + r + 3) * U32 * (np.abs(C).T @ (np.abs(A).T @ np.abs(A)) @ np.abs(C))
    return G, bound, tasks


class _Spy:
    """Counters on the library's own entry points."""
    NAMES = ("svdq_plan_store_gram", "svdq_reconstruct", "svdq_task_reconstruct", "svdq_task_reconstruct_masked")

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


def _plans(bases):
    return {id(rb._batch[0].plan) for b in bases.values() for rb in b.values() if getattr(rb, "_batch", None)}


# ------------------------------------------------------------------------------------------ the Gram, three routes
@pytest.mark.parametrize("world", ["ragged", "plain"])
def test_three_routes_agree_with_the_stored_truth(sq, orc, world, request):
    w = request.getfixturevalue(world)
    art = sq.load_all_artifacts(w["dir"], device="cpu")
    G64, bound, tasks = _stored_truth(art, orc)
    assert tasks == sorted(TASKS)
    lib = sq._native.lib()
    # a fused run's dictionaries
    with _Spy(lib) as calls:
        Gf, tf, rep = sq.task_gram_from_artifacts(w["comp"], w["bases"], device="cuda", basis_report=True)
    n_plans = len(_plans(w["bases"]))
    assert n_plans >= (2 if world == "ragged" else 1)
    assert calls == {"svdq_plan_store_gram": n_plans, "svdq_reconstruct": 0, "svdq_task_reconstruct": 0,
                     "svdq_task_reconstruct_masked": 0}, calls
    # the same store after save -> load -> adopt
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    with _Spy(lib) as calls:
        Ga, ta = sq.task_gram_from_artifacts(ac, ab, device="cuda")
    assert calls["svdq_plan_store_gram"] == len(_plans(ab)) >= 1
    assert calls["svdq_reconstruct"] == calls["svdq_task_reconstruct"] == calls["svdq_task_reconstruct_masked"] == 0
    # un-adopted loaded dictionaries: the per-parameter route
    with _Spy(lib) as calls:
        Gl, tl, rep_l = sq.task_gram_from_artifacts(art["compressed"], art["bases"], device="cuda", basis_report=True)
    assert calls["svdq_plan_store_gram"] == 0 and calls["svdq_reconstruct"] > 0
    assert tf == ta == tl == tasks
    for what, G in (("fused", Gf), ("adopted", Ga), ("loaded", Gl)):
        assert G.dtype == np.float64 and np.array_equal(G, G.T), what
        err = np.abs(G - G64)
        assert (err <= bound).all(), (what, float((err / bound).max()))
    # the orthonormality report names every stored region; the kernel's U^T U (fp32 inside a block) and torch's fp64
    # one differ by at most (256 + r + 3) 2^-24 |U|^T |U|, whose entries are at most the largest diagonal one
    regions = {f"{n} [{r}]" for n, b in art["bases"].items() for r in b if b[r] is not None}
    assert set(rep) == set(rep_l) == regions
    assert all(abs(rep[k] - rep_l[k]) <= (256 + 8 + 3) * U32 * (1.0 + rep_l[k]) for k in rep), (rep, rep_l)


def test_a_lacking_task_counts_as_zeros(sq, ragged):
    """flatten_task_vectors' convention: b3 lacks two of the three equally sized parameters, so its squared norm is about
    a third of a full task's -- in the Gram of the stored vectors as in task_gram of the originals."""
    Gs, tasks = sq.task_gram_from_artifacts(ragged["comp"], ragged["bases"], device="cuda")
    G0, t0 = sq.task_gram(ragged["tv"], device="cuda")
    assert tasks == t0
    i, j = tasks.index(LACKING[0]), tasks.index("b0")
    assert G0[i, i] < 0.5 * G0[j, j] and Gs[i, i] < 0.5 * Gs[j, j]


# ------------------------------------------------------------------------------------------ labels
def _partition(labels):
    groups = {}
    for t, c in labels.items():
        groups.setdefault(c, set()).add(t)
    return {frozenset(m) for m in groups.values()}


@pytest.mark.parametrize("method", ["kmeans", "hierarchical"])
@pytest.mark.parametrize("source", ["fused", "adopted"])
def test_labels_are_those_of_the_original_vectors(sq, plain, method, source):
    bases, comp = plain["bases"], plain["comp"]
    if source == "adopted":
        art = sq.load_all_artifacts(plain["dir"], device="cpu")
        bases, comp = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    got = sq.cluster_tasks_from_artifacts(comp, bases, 2, method=method, device="cuda")
    want = sq.cluster_tasks(plain["tv"], 2, method=method, device="cuda")
    assert _partition(got) == _partition(want) == {frozenset(GROUP_A), frozenset(GROUP_B)}
    with pytest.raises(ValueError):
        sq.cluster_tasks_from_artifacts(comp, bases, 2, method="spectral", device="cuda")


# ------------------------------------------------------------------------------------------ remerge
def _same_state(a, b):
    return list(a) == list(b) and all(_bits(a[n], b[n]) for n in a)


def test_remerge_with_stored_weights_is_reconstruct_from_artifacts(sq, plain):
    want = sq.reconstruct_from_artifacts(plain["dir"], plain["base"], None, device="cuda")["merged_state_dict"]
    res = sq.remerge_from_artifacts(plain["dir"], plain["base"], device="cuda")
    assert res["cluster_assignments"] is None
    assert res["weights"] == sq.load_diagnostics(plain["dir"])["task_weights"]
    assert _same_state(res["merged_state_dict"], want)


def test_remerge_cluster_is_merge_with_clustering_by_hand(sq, plain):
    before = {f: open(os.path.join(plain["dir"], f), "rb").read() for f in ("diagnostics.json", "config.json")}
    res = sq.remerge_from_artifacts(plain["dir"], plain["base"], weighting="cluster", cluster_k=2, device="cuda")
    assign = res["cluster_assignments"]
    assert _partition(assign) == {frozenset(GROUP_A), frozenset(GROUP_B)}
    art = sq.load_all_artifacts(plain["dir"], device="cuda")
    cfg = art["config"]
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    weights = sq.compute_weights(list(art["diagnostics"]["task_weights"]), weighting_strategy="cluster",
                                 temperature=cfg.svd_weighting_temperature, cluster_assignments=assign)
    assert res["weights"] == weights
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    merged = sq.merge_with_clustering(ac, ab, {}, weights, assign, shapes, cfg, device="cuda")
    want = sq.apply_merged_deltas(plain["base"], merged, device="cuda", verbose=False)
    assert _same_state(res["merged_state_dict"], want)
    # another weighting moves the covered tensors, and only those
    uni = sq.remerge_from_artifacts(plain["dir"], plain["base"], weighting="uniform", device="cuda")
    assert uni["weights"] == {t: 1.0 / len(TASKS) for t in TASKS}
    assert _bits(uni["merged_state_dict"]["head.bias"], plain["base"]["head.bias"])
    # the store's files were left alone
    assert not os.path.exists(os.path.join(plain["dir"], "clusters.json"))
    for f, was in before.items():
        assert open(os.path.join(plain["dir"], f), "rb").read() == was
    with pytest.raises(ValueError):
        sq.remerge_from_artifacts(plain["dir"], plain["base"], weighting="best", device="cuda")


# ------------------------------------------------------------------------------------------ scripts
def _run_script(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name), *args], capture_output=True, text=True,
                          timeout=300)


def test_remerge_script_end_to_end(sq, plain, tmp_path):
    store = str(tmp_path / "art")
    shutil.copytree(plain["dir"], store)
    out = str(tmp_path / "merged.pt")
    r = _run_script("remerge.py", "--artifact-dir", store, "--base-model-path", plain["base_path"], "--output-path", out,
                    "--weighting", "cluster", "--cluster-k", "2", "--device", "cuda", "--update-store")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clusters: " in r.stdout
    want = sq.remerge_from_artifacts(plain["dir"], plain["base"], weighting="cluster", cluster_k=2, device="cuda")
    got = torch.load(out, map_location="cpu", weights_only=True)
    assert _same_state(got, want["merged_state_dict"])
    labels = json.load(open(os.path.join(store, "clusters.json")))
    diag = sq.load_diagnostics(store)
    assert labels == diag["cluster_assignments"] and _partition(labels) == _partition(want["cluster_assignments"])
    assert diag["task_weights"] == pytest.approx(want["weights"])
    # the rest of the store is what it was
    for sub in ("basis", "coeffs"):
        for f in os.listdir(os.path.join(store, sub)):
            assert open(os.path.join(store, sub, f), "rb").read() == open(os.path.join(plain["dir"], sub, f), "rb").read()


def test_add_task_script_puts_a_group_a_task_into_group_a(sq, plain, tmp_path):
    store = str(tmp_path / "art")
    shutil.copytree(plain["dir"], store)
    new = str(tmp_path / "new.pt")
    torch.save(plain["ckpt"][NEW], new)
    r = _run_script("add_task.py", "--artifact-dir", store, "--base-model-path", plain["base_path"], "--checkpoint",
                    f"{NEW}={new}", "--weighting", "cluster", "--cluster-k", "2", "--device", "cuda")
    assert r.returncode == 0, r.stdout + r.stderr
    labels = json.load(open(os.path.join(store, "clusters.json")))
    diag = sq.load_diagnostics(store)
    assert labels == diag["cluster_assignments"]
    assert _partition(labels) == {frozenset(GROUP_A + [NEW]), frozenset(GROUP_B)}
    assert set(diag["task_weights"]) == set(TASKS + [NEW])
    # compute_cluster_weights: each cluster's half split evenly over its members
    for t, wt in diag["task_weights"].items():
        assert wt == pytest.approx(0.5 / (5 if t[0] == "a" else 4))
