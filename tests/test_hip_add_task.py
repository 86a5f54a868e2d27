"""
GPU tests of adding a task to a stored artifact set (storage.add_tasks_to_artifacts, compress.project_all_parameters,
driver.adopt_bases): a 3-parameter model with 5 tasks, one parameter masked with a noise region, is compressed and
stored; a sixth checkpoint is then projected onto the stored bases and joins the store.

Tolerance of the comparison with the per-parameter route (``compress_all_parameters`` on the same stored bases): the one
tests/test_hip_parity.py holds the per-call projection to, rtol = 2e-4, atol = 1e-6, on the fp32 values of ``c_high``
plus half an fp16 ulp of each, because ``c_high`` is the fp32 coefficient rounded to fp16 by both routes.
"""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"blk.a": (40, 30), "blk.b": (1027,), "blk.c": (17, 19)}
MASKED = "blk.a"
OLD = [f"t{i}" for i in range(5)]
NEW = "t5"


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.cpu().contiguous().view(w), b.cpu().contiguous().view(w))


@pytest.fixture(scope="module")
def store(sq, tmp_path_factory):
    """The stored 5-task run, the base model, the six checkpoints and the mask; made once, left unchanged."""
    from oracle import svd_hybrid_oracle as orc
    g = torch.Generator().manual_seed(21)
    base, ckpt = {}, {t: {} for t in OLD + [NEW]}
    for j, (name, shape) in enumerate(SHAPES.items()):
        rows = int(np.prod(shape))
        base[name] = torch.randn(shape, generator=g)
        for t, d in zip(OLD + [NEW], orc.synthetic_deltas(rows, 6, 300 + j)):
            ckpt[t][name] = base[name] + d.view(shape)
    base["head.bias"] = torch.randn(7, generator=g)          # a tensor the store does not cover
    for t in ckpt:
        ckpt[t]["head.bias"] = base["head.bias"] + 0.01
    masks = {MASKED: (torch.rand(SHAPES[MASKED], generator=g) < 0.6).cuda()}
    # the task vectors exactly as the from-base route forms them: one fp32 subtraction
    tv = {t: {n: (ckpt[t][n] - base[n]).cuda() for n in SHAPES} for t in OLD + [NEW]}
    cfg = sq.SVDHybridConfig(tasks=list(OLD), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_include_noise=True, svd_noise_shrink=0.5, svd_min_mask_size=10)
    bases, comp = sq.run_basis_and_compress({t: tv[t] for t in OLD}, masks, cfg, "cuda")
    d = str(tmp_path_factory.mktemp("store") / "art")
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()},
            "task_weights": {t: 1.0 / len(OLD) for t in OLD}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    return dict(dir=d, base=base, ckpt=ckpt, masks=masks, tv=tv, cfg=cfg)


def _file_bytes(d, sub):
    out = {}
    for f in sorted(os.listdir(os.path.join(d, sub))):
        with open(os.path.join(d, sub, f), "rb") as fh:
            out[f] = fh.read()
    return out


@pytest.fixture(scope="module")
def added(sq, store, tmp_path_factory):
    """The store with the sixth task added, in a directory of its own, and in place in a copy."""
    import shutil
    out = str(tmp_path_factory.mktemp("added") / "art")
    res = sq.add_tasks_to_artifacts(store["dir"], store["base"], {NEW: store["ckpt"][NEW]}, masks=store["masks"],
                                    output_dir=out, device="cuda")
    inplace = str(tmp_path_factory.mktemp("inplace") / "art")
    shutil.copytree(store["dir"], inplace)
    before = (_file_bytes(inplace, "basis"), open(os.path.join(inplace, "config.json"), "rb").read())
    sq.add_tasks_to_artifacts(inplace, store["base"], {NEW: store["ckpt"][NEW]}, masks=store["masks"], device="cuda")
    return dict(out=out, res=res, inplace=inplace, inplace_before=before)


def _same_artifact(a, b):
    if a is None or b is None:
        return a is None and b is None
    if not _bits(a["c_high_fp16"], b["c_high_fp16"]):
        return False
    qa, qb = a["c_low_quant"], b["c_low_quant"]
    if (qa["num_bits"], qa["num_stages"], tuple(qa["original_shape"]), len(qa["payloads"])) != \
            (qb["num_bits"], qb["num_stages"], tuple(qb["original_shape"]), len(qb["payloads"])):
        return False
    for x, y in zip(qa["payloads"], qb["payloads"]):
        if not (_bits(x["quantized"], y["quantized"]) and _bits(x["scale"].reshape(1), y["scale"].reshape(1))
                and _bits(x["zero_point"].reshape(1), y["zero_point"].reshape(1))):
            return False
    return True


def test_six_tasks_in_the_reference_layout_and_bases_untouched(sq, store, added):
    art0 = sq.load_all_artifacts(store["dir"])
    for d in (added["out"], added["inplace"]):
        art = sq.load_all_artifacts(d)
        assert list(art["diagnostics"]["task_weights"]) == OLD + [NEW]
        assert all(abs(w - 1 / 6) < 1e-12 for w in art["diagnostics"]["task_weights"].values())
        assert sorted(art["compressed"]) == sorted(SHAPES)
        for name in SHAPES:
            per_task = art["compressed"][name]
            assert list(per_task) == OLD + [NEW]
            assert sorted(per_task[NEW]) == (["masked", "unmasked"] if name == MASKED else ["masked"])
            for t in OLD:                                       # the old tasks' artifacts are what they were
                for region, a in art0["compressed"][name][t].items():
                    assert _same_artifact(per_task[t][region], a), (name, t, region)
            for region, b0 in art0["bases"][name].items():      # stored bases: the same tensors, bit for bit
                b1 = art["bases"][name][region]
                assert list(b1) == list(b0)
                for f, v in b0.items():
                    if isinstance(v, torch.Tensor):
                        assert _bits(b1[f], v), (name, region, f)
                    else:
                        assert b1[f] == v, (name, region, f)
    # in place: the basis files and config.json are not rewritten at all
    assert _file_bytes(added["inplace"], "basis") == added["inplace_before"][0]
    assert open(os.path.join(added["inplace"], "config.json"), "rb").read() == added["inplace_before"][1]


def test_new_artifacts_are_project_all_parameters(sq, store, added):
    art = sq.load_all_artifacts(added["out"])
    art0 = sq.load_all_artifacts(store["dir"])
    want = sq.project_all_parameters({NEW: {n: store["ckpt"][NEW][n] for n in SHAPES}}, store["masks"], art0["bases"],
                                     store["cfg"], device="cuda", base_state_dict=store["base"])
    # from checkpoints and from the task vector that holds finetuned - base: the same bits
    want_tv = sq.project_all_parameters({NEW: store["tv"][NEW]}, store["masks"], art0["bases"], store["cfg"], device="cuda")
    assert sorted(want) == sorted(want_tv) == sorted(SHAPES)
    for name in SHAPES:
        for region in ("masked", "unmasked"):
            got = art["compressed"][name][NEW].get(region)
            assert _same_artifact(got, want[name][NEW][region]), (name, region)
            assert _same_artifact(got, want_tv[name][NEW][region]), (name, region)
            assert _same_artifact(got, added["res"]["compressed"][name][NEW][region]), (name, region)


def test_layout_and_c_high_against_the_per_parameter_route(sq, store):
    """project_all_parameters and compress_all_parameters on the same stored bases and the same task vectors: the same
    keys, dtypes and shapes everywhere; c_high within the per-call projection's tolerance."""
    art0 = sq.load_all_artifacts(store["dir"])
    tvs = {t: store["tv"][t] for t in (NEW, OLD[0])}
    a = sq.project_all_parameters(tvs, store["masks"], art0["bases"], store["cfg"], device="cuda")
    b = sq.compress_all_parameters(tvs, store["masks"], art0["bases"], store["cfg"], device="cuda")

    def same_layout(x, y, where):
        assert type(x) is type(y), (where, type(x), type(y))
        if isinstance(x, dict):
            assert list(x) == list(y), (where, list(x), list(y))
            for key in x:
                same_layout(x[key], y[key], where + (key,))
        elif isinstance(x, (list, tuple)) and not isinstance(x, torch.Size):
            assert len(x) == len(y), where
            for i, (u, v) in enumerate(zip(x, y)):
                same_layout(u, v, where + (i,))
        elif isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (where, x.dtype, y.dtype, x.shape, y.shape)
        elif isinstance(x, (int, str, torch.Size)):
            assert x == y, (where, x, y)

    same_layout(a, b, ())
    for name in SHAPES:
        for t in tvs:
            for region in ("masked", "unmasked"):
                x, y = a[name][t][region], b[name][t][region]
                if x is None:
                    continue
                cx, cy = x["c_high_fp16"].float().numpy(), y["c_high_fp16"].float().numpy()
                half_ulp = np.abs(cy) * 2.0 ** -11 + 2.0 ** -25
                assert np.all(np.abs(cx - cy) <= 2e-4 * np.abs(cy) + 1e-6 + half_ulp), (name, t, region)


def test_six_tasks_merge_through_adopted_plans_and_the_new_task_reconstructs(sq, store, added):
    from svdq_amd.driver import LazyArtifacts
    art = sq.load_all_artifacts(added["out"])
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    for name in SHAPES:
        assert isinstance(ac[name], LazyArtifacts) and ac[name]._batch is not None, name
        batch, i = ab[name]["masked"]._batch
        assert batch.plan.N == 6 and batch.task_names[i] == OLD + [NEW]
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    masks = store["masks"]
    every = sq.reconstruct_task_vectors(ac, ab, masks, shapes, art["config"], device="cuda")
    assert list(every) == OLD + [NEW]
    quant = sq.RTVQQuantizer(4, 2)
    for name, shape in SHAPES.items():
        # the new task's own reconstruction is U c + mean of ITS stored coefficients
        regions = {}
        for region, key in (("masked", "masked"), ("noise", "unmasked")):
            a = art["compressed"][name][NEW].get(key)
            if a is None:
                continue
            b = art["bases"][name][region]
            c_low = quant.dequantize(a["c_low_quant"], device="cuda").float()
            regions[region] = sq.reconstruct_from_coefficients(a["c_high_fp16"].cuda().float(), c_low, b["U_high"].cuda(),
                                                               b["U_low"].cuda(), "cuda", mean=b["mean"].cuda())
        if name == MASKED:
            want = sq.reconstruct_from_masked(regions["masked"], regions["noise"] * 0.5, masks[name], torch.Size(shape))
        else:
            want = regions["masked"].view(shape)
        assert _bits(every[NEW][name], want), name
    # the uniform merge of the six-task store is the mean of the six reconstructions
    w = art["diagnostics"]["task_weights"]
    merged = sq.merge_all_parameters(ac, ab, masks, w, shapes, art["config"], device="cuda", verbose=False)
    for name in SHAPES:
        mean6 = sum(every[t][name].double() for t in OLD + [NEW]) / 6
        assert torch.allclose(merged[name].double(), mean6, rtol=1e-4, atol=1e-6), name


def test_reconstruct_from_artifacts_merges_six_tasks_in_two_launches_per_plan(sq, store, tmp_path, monkeypatch):
    """An unmasked store (masks are not stored, so reconstruct_from_artifacts is exact for those only): five tasks
    stored, the sixth added in place, and the reload merges all six through adopted plans -- no per-parameter merge."""
    from svdq_amd import merge as mg
    from svdq_amd.pipeline import CompressPlan
    cfg = sq.SVDHybridConfig(tasks=list(OLD), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress({t: store["tv"][t] for t in OLD}, None, cfg, "cuda")
    d = str(tmp_path / "art")
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()},
            "task_weights": {t: 0.2 for t in OLD}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    res = sq.add_tasks_to_artifacts(d, store["base"], {NEW: store["ckpt"][NEW]}, device="cuda")
    assert res["tasks"] == OLD + [NEW] and res["output_dir"] == d
    calls = []
    real = CompressPlan.merge
    monkeypatch.setattr(CompressPlan, "merge", lambda self, *a, **k: (calls.append(self.N), real(self, *a, **k))[1])

    def no_per_parameter_route(*a, **k):
        raise AssertionError("merge_parameter was called: a parameter left the adopted route")
    monkeypatch.setattr(mg, "merge_parameter", no_per_parameter_route)
    base = {n: v.cuda() for n, v in store["base"].items()}
    out = sq.reconstruct_from_artifacts(d, base, device="cuda")
    assert calls == [6]                                            # one plan of six tasks, one svdq_merge
    assert list(out["diagnostics"]["task_weights"]) == OLD + [NEW]
    monkeypatch.undo()
    art = sq.load_all_artifacts(d)
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    every = sq.reconstruct_task_vectors(ac, ab, {}, shapes, art["config"], device="cuda")
    merged = out["merged_state_dict"]
    for name in SHAPES:
        mean6 = sum(every[t][name].double() for t in OLD + [NEW]) / 6
        got = merged[name].double() - base[name].double()
        assert torch.allclose(got, mean6, rtol=1e-4, atol=2e-6), name
    assert _bits(merged["head.bias"], base["head.bias"])


def test_refusals(sq, store, tmp_path):
    with pytest.raises(ValueError, match="already"):
        sq.add_tasks_to_artifacts(store["dir"], store["base"], {OLD[2]: store["ckpt"][NEW]}, masks=store["masks"],
                                  output_dir=str(tmp_path / "x"))
    many = {f"n{i}": store["ckpt"][NEW] for i in range(28)}      # 5 + 28 = 33
    with pytest.raises(ValueError, match="32"):
        sq.add_tasks_to_artifacts(store["dir"], store["base"], many, masks=store["masks"], output_dir=str(tmp_path / "y"))
    assert not os.path.exists(tmp_path / "x") and not os.path.exists(tmp_path / "y")
    art0 = sq.load_all_artifacts(store["dir"])
    with pytest.raises(ValueError, match="blk.a"):               # without the mask the selected count is not the stored D
        sq.project_all_parameters({NEW: store["tv"][NEW]}, {}, art0["bases"], store["cfg"], device="cuda")
    with pytest.raises(ValueError, match="32"):
        sq.project_all_parameters({f"n{i}": store["tv"][NEW] for i in range(33)}, store["masks"], art0["bases"],
                                  store["cfg"], device="cuda")
