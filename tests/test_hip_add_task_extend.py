"""
GPU tests of adding a task to a stored artifact set WITH the basis extension (storage.add_tasks_to_artifacts(...,
extend_basis=True), compress.extend_bases): the five-task store of tests/test_hip_add_task.py's kind -- a 3-parameter
model, one parameter masked with a noise region -- and a sixth checkpoint that is added once plainly and once with
``extend_basis=True``, each into a directory of its own.

The sixth task's error.  For every extended entry, with u_Q = 2^-11 (the stored bases are fp16) and one new task (M = 1):
    |xc - U c - Q d|_2  <=  u_Q | |Q||d| |_2 + fp32 terms + min_residual sqrt(M) |xc|         (tests/test_hip_extend_basis.py, 3)
and the stored artifact adds the rounding of c_high' to fp16, u_Q | |U_high'||c_high'| |_2, and the quantization of
c_low: the last RTVQ stage rounds to the nearest code and dequantizes as (q - zp) / scale, so each element is off by at
most 1 / (2 scale_last) -- computed here from the stored scales -- which moves the reconstruction by at most
| |U_low| |_2 sqrt(n_low) / (2 scale_last).  The fp32
terms are computed as that file derives them: de = (r + 2) 2^-24 (|xc| + |U||c|) per element of e, 2 |de|_2 for the
one new task, and (M + 4) 2^-24 |e|_2 for the chain over the slots.
"""

import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"blk.a": (40, 30), "blk.b": (1027,), "blk.c": (17, 19)}
MASKED = "blk.a"
OLD = [f"t{i}" for i in range(5)]
NEW = "t5"
UQ = 2.0 ** -11
U32 = 2.0 ** -24
MINRES = 2.0 ** -12


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


def _file_bytes(d, sub):
    out = {}
    for f in sorted(os.listdir(os.path.join(d, sub))):
        with open(os.path.join(d, sub, f), "rb") as fh:
            out[f] = fh.read()
    return out


def _make_world(sq, tmp_path_factory, center):
    from oracle import svd_hybrid_oracle as orc
    g = torch.Generator().manual_seed(21)
    base, ckpt = {}, {t: {} for t in OLD + [NEW]}
    for j, (name, shape) in enumerate(SHAPES.items()):
        rows = int(np.prod(shape))
        base[name] = torch.randn(shape, generator=g)
        for t, d in zip(OLD + [NEW], orc.synthetic_deltas(rows, 6, 300 + j)):
            ckpt[t][name] = base[name] + d.view(shape)
    masks = {MASKED: (torch.rand(SHAPES[MASKED], generator=g) < 0.6).cuda()}
    tv = {t: {n: (ckpt[t][n] - base[n]).cuda() for n in SHAPES} for t in OLD + [NEW]}
    cfg = sq.SVDHybridConfig(tasks=list(OLD), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_include_noise=True, svd_noise_shrink=0.5, svd_min_mask_size=10,
                             svd_center=center)
    bases, comp = sq.run_basis_and_compress({t: tv[t] for t in OLD}, masks, cfg, "cuda")
    d = str(tmp_path_factory.mktemp("store") / "art")
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()},
            "task_weights": {t: 1.0 / len(OLD) for t in OLD}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    plain = str(tmp_path_factory.mktemp("plain") / "art")
    sq.add_tasks_to_artifacts(d, base, {NEW: ckpt[NEW]}, masks=masks, output_dir=plain, device="cuda")
    off = str(tmp_path_factory.mktemp("off") / "art")
    sq.add_tasks_to_artifacts(d, base, {NEW: ckpt[NEW]}, masks=masks, output_dir=off, device="cuda", extend_basis=False)
    ext = str(tmp_path_factory.mktemp("ext") / "art")
    res = sq.add_tasks_to_artifacts(d, base, {NEW: ckpt[NEW]}, masks=masks, output_dir=ext, device="cuda",
                                    extend_basis=True)
    return dict(dir=d, base=base, ckpt=ckpt, masks=masks, tv=tv, cfg=cfg, plain=plain, off=off, ext=ext, res=res)


@pytest.fixture(scope="module")
def world(sq, tmp_path_factory):
    """The stored 5-task run and the sixth task added plainly and with the extension; made once, left unchanged."""
    return _make_world(sq, tmp_path_factory, True)


@pytest.fixture(scope="module")
def world_nc(sq, tmp_path_factory):
    """The same on a store without a mean (svd_center off)."""
    return _make_world(sq, tmp_path_factory, False)


def _regions(name):
    return [("masked", "masked"), ("noise", "unmasked")] if name == MASKED else [("masked", "masked")]


def _xc(world, name, region, basis):
    x = world["tv"][NEW][name].cpu()
    if name == MASKED:
        m = world["masks"][name].cpu()
        x = x[m] if region == "masked" else x[~m]
    x = x.reshape(-1).float()
    return (x - basis["mean"].reshape(-1).float()).double() if basis.get("mean") is not None else x.double()


def test_extend_basis_false_writes_the_plain_files(world):
    assert _file_bytes(world["off"], "coeffs") == _file_bytes(world["plain"], "coeffs")
    assert _file_bytes(world["off"], "basis") == _file_bytes(world["plain"], "basis")
    dg = json.load(open(os.path.join(world["off"], "diagnostics.json")))
    assert "captured_energy" not in dg and "columns" not in dg


def test_store_loads_adopts_and_merges_six_tasks(sq, world):
    from svdq_amd.driver import LazyArtifacts
    art = sq.load_all_artifacts(world["ext"])
    assert list(art["diagnostics"]["task_weights"]) == OLD + [NEW]
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    for name in SHAPES:
        assert isinstance(ac[name], LazyArtifacts) and ac[name]._batch is not None, name
        batch, i = ab[name]["masked"]._batch
        assert batch.plan.N == 6 and batch.task_names[i] == OLD + [NEW]
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    every = sq.reconstruct_task_vectors(ac, ab, world["masks"], shapes, art["config"], device="cuda")
    w = art["diagnostics"]["task_weights"]
    merged = sq.merge_all_parameters(ac, ab, world["masks"], w, shapes, art["config"], device="cuda", verbose=False)
    for name in SHAPES:
        mean6 = sum(every[t][name].double() for t in OLD + [NEW]) / 6
        assert torch.allclose(merged[name].double(), mean6, rtol=1e-4, atol=1e-6), name


def test_nothing_old_moves(sq, world):
    """Stored columns, U_low, mean and the old tasks' c_low are the stored bytes; c_high is zero-padded; and every old
    task reconstructs to the same values from the extended store (torch.equal: the fma chain only meets zeros, and a
    -0 may become +0)."""
    art0 = sq.load_all_artifacts(world["dir"])
    art = sq.load_all_artifacts(world["ext"])
    cols = world["res"]["columns"]
    assert sum(cols.values()) > 0
    for name in SHAPES:
        for region, key in _regions(name):
            b0, b1 = art0["bases"][name][region], art["bases"][name][region]
            m = cols[f"{name} [{region}]"]
            k = int(b0["k"])
            assert int(b1["k"]) == k + m and b1["U_high"].shape == (b0["U_high"].shape[0], k + m)
            assert _bits(b1["U_high"][:, :k].contiguous(), b0["U_high"].contiguous())
            assert _bits(b1["U_low"], b0["U_low"]) and _bits(b1["mean"], b0["mean"])
            sv0, sv1 = b0["singular_values"].float(), b1["singular_values"].float()
            assert torch.equal(sv1[:k], sv0[:k]) and torch.equal(sv1[k + m:], sv0[k:])
            if m:
                assert int(b1["N"]) == int(b0["N"]) + 1
            for t in OLD:
                a0, a1 = art0["compressed"][name][t][key], art["compressed"][name][t][key]
                assert _bits(a1["c_high_fp16"][:k].contiguous(), a0["c_high_fp16"]) and not a1["c_high_fp16"][k:].any()
                assert a1["c_high_fp16"].numel() == k + m
                for x, y in zip(a0["c_low_quant"]["payloads"], a1["c_low_quant"]["payloads"]):
                    assert _bits(x["quantized"], y["quantized"]) and _bits(x["scale"].reshape(1), y["scale"].reshape(1))
                    assert _bits(x["zero_point"].reshape(1), y["zero_point"].reshape(1))
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    ab0, ac0 = sq.adopt_artifacts(art0["bases"], art0["compressed"], art0["config"], device="cuda")
    ab1, ac1 = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    r0 = sq.reconstruct_task_vectors(ac0, ab0, world["masks"], shapes, art0["config"], device="cuda")
    r1 = sq.reconstruct_task_vectors(ac1, ab1, world["masks"], shapes, art["config"], tasks=OLD, device="cuda")
    for t in OLD:
        for name in SHAPES:
            assert torch.equal(r0[t][name], r1[t][name]), (t, name)


def _sixth_task(sq, world):
    """Per extended entry, in fp64 from the stored artifacts: |xc - U' c'| of the sixth task on the plain and on the
    extended store, and the bound of the module docstring.  Returns (arts, errs, bounds, evals); evals[entry]: what an
    fp32 evaluation of x - U' c' (the diagnostics kernel's fma chain over the r' columns) may add to the norm,
    (r' + 2) u (|x| + | |U'||c'| |), x the uncentred delta the diagnostics compare against."""
    quant = sq.RTVQQuantizer(4, 2)
    arts = {w: sq.load_all_artifacts(world[w]) for w in ("plain", "ext")}
    cols = world["res"]["columns"]
    errs, bounds, evals = {}, {}, {}
    for name in SHAPES:
        for region, key in _regions(name):
            if cols[f"{name} [{region}]"] == 0:
                continue
            err = {}
            for w, art in arts.items():
                b, a = art["bases"][name][region], art["compressed"][name][NEW][key]
                xc = _xc(world, name, region, b)
                c_low = quant.dequantize(a["c_low_quant"], device="cpu").double().reshape(-1)
                c = torch.cat([a["c_high_fp16"].double().reshape(-1), c_low])
                Uall = torch.cat([b["U_high"].double(), b["U_low"].double()], dim=1)
                err[w] = float((xc - Uall @ c).norm())
                if w == "ext":
                    k1, n_low = int(b["k"]), int(b["U_low"].shape[1])
                    pays = a["c_low_quant"]["payloads"]
                    step = 0.5 / float(pays[-1]["scale"]) if n_low and pays else 0.0      # dequantization: (q - zp) / scale
                    qlow = float(torch.linalg.matrix_norm(b["U_low"].double().abs(), 2)) * np.sqrt(n_low) * step \
                        if n_low else 0.0
                    chigh = UQ * float((b["U_high"].double().abs() @ a["c_high_fp16"].double().abs()).norm())
                    xn = float(xc.norm())
                    # the fp32 terms, as tests/test_hip_extend_basis.py derives them, from the STORED columns (the
                    # first k' - m of U_high', and U_low).  The kernel's fp32 c is a dot product of D terms: within
                    # (D + 2) u |U|^T |xc| of the fp64 one, in whatever order it is summed.
                    m = cols[f"{name} [{region}]"]
                    Uold = torch.cat([b["U_high"][:, :k1 - m].double(), b["U_low"].double()], dim=1)
                    r, D = Uold.shape[1], Uold.shape[0]
                    c64 = Uold.T @ xc
                    cabs = c64.abs() + (D + 2) * U32 * (Uold.abs().T @ xc.abs())
                    de = (r + 2) * U32 * (xc.abs() + Uold.abs() @ cabs)          # per element of e
                    e = xc - Uold @ c64
                    # M = 1: |de_j|_2 + |de|_F = 2 |de|_2; the chain over the slots with |z||d| = 1: (M + 4) u |e|_2
                    fp32 = 2 * float(de.norm()) + (1 + 4) * U32 * float(e.norm())
                    bounds[(name, region)] = 2 * chigh + fp32 + MINRES * xn + qlow
                    mn = float(b["mean"].double().norm()) if b.get("mean") is not None else 0.0      # |x| <= |xc| + |mean|
                    evals[(name, region)] = (Uall.shape[1] + 2) * U32 * (xn + mn + float((Uall.abs() @ c.abs()).norm()))
            errs[(name, region)] = err
            print(name, region, "plain", err["plain"], "extended", err["ext"], "bound", bounds[(name, region)])
    return arts, errs, bounds, evals


def _relative_errors(sq, world, arts):
    """The sixth task's relative_error per parameter (of a masked parameter: its masked region, which is what the
    diagnostics compare) on the plain and on the extended store."""
    rel = {}
    for w, art in arts.items():
        ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda",
                                    masks=world["masks"])
        dg = sq.compute_all_diagnostics_from_checkpoints(world["base"], {t: world["ckpt"][t] for t in OLD + [NEW]}, ac,
                                                         ab, world["masks"], art["config"], device="cuda")
        rel[w] = {n: _task_rel(dg["per_parameter"][n], NEW) for n in SHAPES}
    print("relative_error of the sixth task", rel)
    return rel


def _x_norm(world, name):
    x = world["tv"][NEW][name].cpu()
    if name == MASKED:
        x = x[world["masks"][name].cpu()]
    return float(x.double().norm())


def test_the_sixth_task_is_reconstructed(sq, world):
    """Per extended entry, in fp64 from the stored artifacts: |xc - U' c'| within the bound of the module docstring, and
    the plain route's error at least 10 x that.  Then the number users see on this CENTRED store: the reference's
    diagnostics reconstruct WITHOUT the mean and compare against the uncentred delta (a quirk this package keeps,
    diagnostics.py), so here relative_error <= (bound + |mean|) / |x|; test_relative_error_without_a_mean asserts the
    bound alone."""
    arts, errs, bounds, evals = _sixth_task(sq, world)
    assert bounds
    for key, err in errs.items():
        assert err["ext"] <= bounds[key], (key, err, bounds[key])
        assert err["plain"] >= 10 * err["ext"], (key, err)
    rel = _relative_errors(sq, world, arts)
    for n in SHAPES:
        assert rel["ext"][n] < rel["plain"][n], (n, rel)
        if (n, "masked") in bounds:
            mean = float(arts["ext"]["bases"][n]["masked"]["mean"].double().norm())
            lim = (bounds[(n, "masked")] + mean + evals[(n, "masked")]) / _x_norm(world, n)
            assert rel["ext"][n] <= lim, (n, rel["ext"][n], lim)


def test_relative_error_without_a_mean(sq, world_nc):
    """On a store without a mean the diagnostics' reconstruction is the whole one, and the sixth task's relative_error
    drops from the plain route's value to below the bound plus its c_low quantization step (both inside ``bounds``),
    over |x| -- for every parameter, the masked one by its masked region.  The diagnostics evaluate x - U' c' in fp32:
    ``evals`` is what that may add."""
    world = world_nc
    arts, errs, bounds, evals = _sixth_task(sq, world)
    assert all(b["masked"].get("mean") is None for b in arts["ext"]["bases"].values())
    assert all((n, "masked") in bounds for n in SHAPES)
    for key, err in errs.items():
        assert err["ext"] <= bounds[key], (key, err, bounds[key])
        assert err["plain"] >= 10 * err["ext"], (key, err)
    rel = _relative_errors(sq, world, arts)
    for n in SHAPES:
        xn = _x_norm(world, n)
        lim = (bounds[(n, "masked")] + evals[(n, "masked")]) / xn
        print(n, "relative_error plain", rel["plain"][n], "extended", rel["ext"][n], "bound", lim)
        assert rel["ext"][n] <= lim, (n, rel["ext"][n], lim)
        assert rel["plain"][n] >= 10 * rel["ext"][n], (n, rel)


def _task_rel(per_param, task):
    """The task's relative_error out of one parameter's diagnostics dictionary, wherever the layout keeps it."""
    found = []

    def walk(d, under_task):
        if isinstance(d, dict):
            for key, v in d.items():
                if key == "relative_error" and under_task and isinstance(v, float):
                    found.append(v)
                else:
                    walk(v, under_task or key == task)

    walk(per_param, False)
    assert found, (task, list(per_param))
    return max(found)


def test_captured_energy_is_reported(sq, world):
    """captured_energy = 1 - sum |e|^2 / sum |xc|^2 over the batched entries, e the residual against the STORED columns;
    the model: fp64, from the stored bases and the fp32 coefficients' definition c = U^T xc."""
    dg = json.load(open(os.path.join(world["ext"], "diagnostics.json")))
    assert list(dg["captured_energy"]) == [NEW] and dg["captured_energy"] == world["res"]["captured_energy"]
    assert dg["columns"] == world["res"]["columns"] and set(dg["columns"]) == {
        f"{n} [{r}]" for n in SHAPES for r, _ in _regions(n)}
    art0 = sq.load_all_artifacts(world["dir"])
    e2 = x2 = 0.0
    for name in SHAPES:
        for region, key in _regions(name):
            b = art0["bases"][name][region]
            xc = _xc(world, name, region, b)
            Uall = torch.cat([b["U_high"].double(), b["U_low"].double()], dim=1)
            e = xc - Uall @ (Uall.T @ xc)
            e2 += float(e @ e)
            x2 += float(xc @ xc)
    assert abs(dg["captured_energy"][NEW] - (1 - e2 / x2)) <= 1e-6


def _same_tree(a, b, where=""):
    """Two artifact dictionaries are the same: keys, types, scalars, and tensors bit for bit."""
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (where, list(a), list(b))
        for key in a:
            _same_tree(a[key], b[key], f"{where}/{key}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f"{where}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert _bits(a, b), where
    else:
        assert a == b or (a != a and b != b), (where, a, b)


def test_a_task_in_the_span_gets_the_plain_dictionaries(sq, world):
    """A new task built as mean + U a in every region: m = 0 everywhere, and what extend_bases returns for it is what
    project_all_parameters returns -- the artifacts bit for bit, the bases the very objects that came in."""
    art0 = sq.load_all_artifacts(world["dir"])
    g = torch.Generator().manual_seed(5)
    x = {}
    for name, shape in SHAPES.items():
        full = torch.zeros(shape)
        for region, _ in _regions(name):
            b = art0["bases"][name][region]
            U = torch.cat([b["U_high"].double(), b["U_low"].double()], dim=1)
            mean = b["mean"].double().reshape(-1)
            # "in the span" for the kernel means e = xc - U (U^T xc) = U (I - U^T U) a = 0, which needs U^T U a = a: a is
            # taken from the eigenvectors of U^T U whose eigenvalue is within 1e-4 of 1, the rounding of the stored fp16
            # columns.  (A centred store of N tasks has rank N - 1; where r = N the last stored column belongs to a
            # singular value near 0 and is orthonormal to 2 - 4e-4 only, which is above min_residual = 2.4e-4.)
            ev, V = torch.linalg.eigh(U.T @ U)
            good = V[:, (ev - 1).abs() <= 1e-4]
            print(name, region, "eigenvalues of U^T U - 1", (ev - 1).tolist())
            assert good.shape[1] >= 1, (name, region, ev)
            a = good @ torch.randn(good.shape[1], generator=g, dtype=torch.float64) * max(1.0, float(mean.norm()))
            v = (mean + U @ a).float()
            if name == MASKED:
                m = world["masks"][name].cpu()
                full[m if region == "masked" else ~m] = v
            else:
                full = v.view(shape)
        x[name] = full.cuda()
    args = ({"span": x}, world["masks"], art0["bases"], art0["config"])
    plain = sq.project_all_parameters(*args, device="cuda")
    res = sq.extend_bases(*args, device="cuda")
    assert set(res["columns"]) == {(n, r) for n in SHAPES for r, _ in _regions(n)}
    assert not any(res["columns"].values()) and res["skipped"] == []
    _same_tree(res["compressed"], plain, "compressed")
    assert list(res["bases"]) == list(art0["bases"])
    for name in SHAPES:
        assert res["bases"][name] is art0["bases"][name], name
    assert res["captured_energy"]["span"] >= 1.0 - 1e-6


def test_in_place_writes_the_same_store(sq, world, tmp_path):
    """In place only the coefficient files, diagnostics.json and the basis files of extended parameters are rewritten:
    the result is the store the out-of-place call wrote, file for file."""
    import shutil
    d = str(tmp_path / "art")
    shutil.copytree(world["dir"], d)
    cfg_before = open(os.path.join(d, "config.json"), "rb").read()
    res = sq.add_tasks_to_artifacts(d, world["base"], {NEW: world["ckpt"][NEW]}, masks=world["masks"], device="cuda",
                                    extend_basis=True)
    assert res["output_dir"] == d and res["columns"] == world["res"]["columns"]
    a, b = sq.load_all_artifacts(d), sq.load_all_artifacts(world["ext"])
    for name in SHAPES:
        for region, key in _regions(name):
            for f in ("U_high", "U_low", "mean", "singular_values"):
                assert _bits(a["bases"][name][region][f], b["bases"][name][region][f]), (name, region, f)
            assert a["bases"][name][region]["k"] == b["bases"][name][region]["k"]
            for t in OLD + [NEW]:
                assert _bits(a["compressed"][name][t][key]["c_high_fp16"], b["compressed"][name][t][key]["c_high_fp16"])
    assert a["diagnostics"]["captured_energy"] == b["diagnostics"]["captured_energy"]
    assert open(os.path.join(d, "config.json"), "rb").read() == cfg_before


def test_refusals(sq, world, tmp_path):
    many = {f"n{i}": world["ckpt"][NEW] for i in range(9)}
    with pytest.raises(ValueError, match="1 to 8 new tasks"):
        sq.add_tasks_to_artifacts(world["dir"], world["base"], many, masks=world["masks"], output_dir=str(tmp_path / "x"),
                                  extend_basis=True)
    assert not os.path.exists(tmp_path / "x")
