"""
GPU tests of consolidating a stored artifact set (storage.consolidate_artifacts, compress.consolidate_bases): the
five-task store of tests/test_hip_add_task_extend.py's kind -- a 3-parameter model, one parameter masked with a noise
region -- grown by a sixth task with ``extend_basis=True`` and then consolidated, each store in a directory of its own.

The bound on what consolidation may move.  Per region and task, from the STORED artifacts of both stores alone, in fp64:
with A = [U_high | U_low | mean] and b_j = [c_j ; 1] of the old store (c_j = fp16 c_high, dequantized c_low), and U', mean',
sigma', cq' (the stored fp16 / dequantized coefficients) of the new one,
    | (U' cq' + mean') - A b_j |_2  <=  | rounding + quantization |_2 + chain + sqrt(dropped_energy + eta) + evaluation
  rounding      U' is the fp16 rounding of A W: per element 2^-11 (1 + 2^-10) |u'| (2^-25 below the normal range), times |c'|,
                |c'| <= |cq'| + step
  quantization  |U'| step, step = what fp16 (c_high: 2^-11 |c|, 2^-25) and the RTVQ (c_low: one step of the last stage,
                1 / scale_last, plus 2^-21 of the stage values for the fp32 operations) may have moved c' by
  chain         the rebase pass forms A [W | bbar] as fp32 fma chains of r + 1 terms over fp32 W, bbar:
                (r + 3) 2^-24 | |A| (|W| |c'| + |bbar|) |_2 <= (r + 3) 2^-24 ||A||_F (||W||_F |c'|_2 + |bbar|_2), and
                W = Bc V Sigma^-1 has ||W||_F^2 <= ||Bc||_2^2 sum_i 1 / sigma'_i^2  (Bc = B - bbar 1^T from the old store)
  dropped       the directions below the noise floor: sqrt(dropped_energy + eta), both recorded in diagnostics.json
  evaluation    both reconstructions compared are formed by fp32 fma chains: (r + 3) 2^-24 | |A| |b_j| |_2 and
                (r' + 3) 2^-24 | |U'| |cq'| + |mean'| |_2.
A masked parameter's delta is its two regions scattered (the noise region times svd_noise_shrink <= 1): the bounds add.
"""

import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, artifact_manifest

pytestmark = pytest.mark.gpu

SHAPES = {"blk.a": (40, 30), "blk.b": (1027,), "blk.c": (17, 19)}
MASKED = "blk.a"
OLD = [f"t{i}" for i in range(5)]
NEW = "t5"
ALL = OLD + [NEW]
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.fixture(scope="module")
def world(sq, tmp_path_factory):
    """The stored 5-task run, the sixth task added with the extension, and that store consolidated; made once."""
    from oracle import svd_hybrid_oracle as orc
    g = torch.Generator().manual_seed(21)
    base, ckpt = {}, {t: {} for t in ALL}
    for j, (name, shape) in enumerate(SHAPES.items()):
        rows = int(np.prod(shape))
        base[name] = torch.randn(shape, generator=g)
        for t, d in zip(ALL, orc.synthetic_deltas(rows, 6, 300 + j)):
            ckpt[t][name] = base[name] + d.view(shape)
    masks = {MASKED: (torch.rand(SHAPES[MASKED], generator=g) < 0.6).cuda()}
    tv = {t: {n: (ckpt[t][n] - base[n]).cuda() for n in SHAPES} for t in OLD}
    cfg = sq.SVDHybridConfig(tasks=list(OLD), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_include_noise=True, svd_noise_shrink=0.5, svd_min_mask_size=10,
                             svd_center=True)
    bases, comp = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    d = str(tmp_path_factory.mktemp("store") / "art")
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()},
            "task_weights": {t: 1.0 / len(OLD) for t in OLD}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d)
    ext = str(tmp_path_factory.mktemp("ext") / "art")
    sq.add_tasks_to_artifacts(d, base, {NEW: ckpt[NEW]}, masks=masks, output_dir=ext, device="cuda", extend_basis=True)
    con = str(tmp_path_factory.mktemp("con") / "art")
    res = sq.consolidate_artifacts(ext, output_dir=con)
    return dict(dir=d, base=base, ckpt=ckpt, masks=masks, cfg=cfg, ext=ext, con=con, res=res)


def _regions(name):
    return [("masked", "masked"), ("noise", "unmasked")] if name == MASKED else [("masked", "masked")]


def _coeffs(sq, art, key, k, n_low):
    """(cq [r] fp64, step [r]): the stored coefficients and what rounding / quantization may have moved them by."""
    quant = sq.RTVQQuantizer(4, 2)
    ch = art[key]["c_high_fp16"].double().reshape(-1).numpy()
    q = art[key]["c_low_quant"]
    cl = quant.dequantize(q, device="cpu").double().reshape(-1).numpy() if n_low else np.zeros(0)
    assert ch.size == k and cl.size == n_low and np.isfinite(cl).all()
    step_h = np.maximum(2.0 ** -11 * np.abs(ch), 2.0 ** -25)
    if n_low:
        scales = np.array([float(p["scale"]) for p in q["payloads"]])
        step_l = (1 + 2.0 ** -20) / scales[-1] + 2.0 ** -21 * (np.abs(cl) + (2.0 ** int(q["num_bits"]) / scales).sum())
    else:
        step_l = np.zeros(0)
    return np.concatenate([ch, cl]), np.concatenate([step_h, step_l * np.ones(n_low)])


def _region_arrays(sq, art, name, region, key, tasks):
    b = art["bases"][name][region]
    k, n_low = int(b["k"]), int(b["U_low"].shape[1])
    U = torch.cat([b["U_high"].double(), b["U_low"].double()], dim=1).numpy()
    mean = b["mean"].double().reshape(-1).numpy() if b.get("mean") is not None else None
    C, S = {}, {}
    for t in tasks:
        a = art["compressed"][name].get(t)
        if a is not None and a.get(key) is not None:
            C[t], S[t] = _coeffs(sq, a, key, k, n_low)
    return b, U, mean, C, S


def _bound(sq, old, new, diag_new, name, region, key, tasks):
    """({task: bound}, {task: its evaluation term}) of the module docstring for one region."""
    b0, U0, m0, C0, _ = _region_arrays(sq, old, name, region, key, tasks)
    b1, U1, m1, C1, S1 = _region_arrays(sq, new, name, region, key, tasks)
    have = [t for t in tasks if t in C0]
    assert sorted(C1) == sorted(have)
    A = U0 if m0 is None else np.concatenate([U0, m0[:, None]], axis=1)
    B = np.stack([np.concatenate([C0[t], [1.0]]) if m0 is not None else C0[t] for t in have], axis=1)
    bbar = B.mean(axis=1) if m1 is not None else np.zeros(B.shape[0])
    Bc = B - bbar[:, None]
    r, r1 = U0.shape[1], U1.shape[1]
    sig = b1["singular_values"].double().numpy()[:r1]
    w_f = np.linalg.norm(Bc, 2) * np.sqrt((1.0 / sig ** 2).sum()) * (1 + 2.0 ** -20) if r1 else 0.0
    tag = f"{name} [{region}]"
    slack = np.sqrt(diag_new["dropped_energy"][tag] + diag_new["noise_floor"][tag])
    rel16 = 2.0 ** -11 * (1 + 2.0 ** -10) if b1["U_high"].dtype is torch.float16 else 0.0
    sub16 = 2.0 ** -25 if rel16 else 0.0
    out, evs = {}, {}
    for j, t in enumerate(have):
        cq, step = C1[t], S1[t]
        cabs = np.abs(cq) + step
        pre = A @ B[:, j]
        post = U1 @ cq + (m1 if m1 is not None else 0.0)
        elem = (rel16 * np.abs(U1) + sub16) @ cabs + np.abs(U1) @ step
        chain = (r + 3) * U32 * np.linalg.norm(A) * (w_f * np.linalg.norm(cabs) + np.linalg.norm(bbar))
        ev = (r + 3) * U32 * np.linalg.norm(np.abs(A) @ np.abs(B[:, j])) + \
            (r1 + 3) * U32 * np.linalg.norm(np.abs(U1) @ np.abs(cq) + (np.abs(m1) if m1 is not None else 0.0))
        out[t] = np.linalg.norm(elem) + chain + slack + ev
        evs[t] = ev
        assert np.linalg.norm(post - pre) <= np.linalg.norm(elem) + chain + slack, (tag, t)      # the fp64 statement
    return out, evs


def _reconstruct(sq, world, d, tasks=None):
    art = sq.load_all_artifacts(d)
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda", masks=world["masks"])
    shapes = {n: torch.Size(s) for n, s in SHAPES.items()}
    rec = sq.reconstruct_task_vectors(ac, ab, world["masks"], shapes, art["config"], tasks=tasks, device="cuda")
    w = art["diagnostics"]["task_weights"]
    merged = sq.merge_all_parameters(ac, ab, world["masks"], w, shapes, art["config"], device="cuda", verbose=False)
    return art, rec, merged


def test_extend_then_consolidate(sq, world):
    ext, rec0, mer0 = _reconstruct(sq, world, world["ext"])
    con, rec1, mer1 = _reconstruct(sq, world, world["con"])
    dg = con["diagnostics"]
    assert dg["tasks"] == ALL and list(dg["task_weights"]) == ALL and world["res"]["skipped"] == []
    total = {t: {n: 0.0 for n in SHAPES} for t in ALL}
    evals = {t: {n: 0.0 for n in SHAPES} for t in ALL}
    for name in SHAPES:
        for region, key in _regions(name):
            b0, b1 = ext["bases"][name][region], con["bases"][name][region]
            sv = b1["singular_values"].float()
            r0 = int(b0["k"]) + int(b0["U_low"].shape[1])
            r1 = int(b1["k"]) + int(b1["U_low"].shape[1])
            assert sv.numel() == r1 and bool((sv[1:] <= sv[:-1]).all()), (name, region, sv)      # descending again
            assert int(b1["N"]) == 6 and 1 <= r1 <= 5 and r1 <= r0, (name, region, r0, r1)
            assert dg["columns"][f"{name} [{region}]"] == [r0, r1]
            assert 1 <= int(b1["k"]) <= r1 and b1["mean"] is not None
            bounds, evs = _bound(sq, ext, con, dg, name, region, key, ALL)
            for t in ALL:
                total[t][name] += bounds[t]
                evals[t][name] += evs[t]
    for t in ALL:
        for name in SHAPES:
            diff = float((rec1[t][name].double() - rec0[t][name].double()).norm())
            print(t, name, "moved", diff, "bound", total[t][name])
            assert diff <= total[t][name], (t, name, diff, total[t][name])
    # the merge of both stores (remerge_from_artifacts' own lines, with the masks the store was written with: masks are
    # not stored) agrees within the weighted sum of those bounds
    w0, w1 = ext["diagnostics"]["task_weights"], dg["task_weights"]
    assert w0 == w1
    for name in SHAPES:
        # a merge reconstructs from the weighted coefficients: its own fma chains are within the weighted evaluation
        # terms again (|U| |sum w c| <= sum w |U| |c|), and so are the fp32 roundings of the weighted sums (N + 2 <= r + 3)
        lim = sum(w1[t] * (total[t][name] + 2 * evals[t][name]) for t in ALL)
        diff = float((mer1[name].double() - mer0[name].double()).norm())
        assert diff <= lim, (name, diff, lim)


def test_drop_a_task_then_add_it_again(sq, world, tmp_path):
    """consolidate_artifacts(tasks=five of six) and add_tasks_to_artifacts of the dropped one again: the sequence the
    feature exists for.  The dropped task is in no file; the kept tasks stay within the bound; the store takes the task
    back, extended, and reconstructs six tasks.  Run with the store's own settings (4 bits, two stages).  Five centred
    tasks leave r' = 4 and, where the rank rule gives k' = 2, a c_low of two elements, whose second quantizer stage has
    no range more often than not (scale = 1 / 0, NaN behind it): such a region is stored on the high side and listed
    under ``promoted``, and every kept task's stored coefficients and reconstruction are finite."""
    five = str(tmp_path / "five")
    keep = [t for t in ALL if t != "t2"]
    res = sq.consolidate_artifacts(world["ext"], output_dir=five, tasks=keep)
    assert sq.load_config(five).svd_rtvq_stages == 2
    assert res["tasks"] == keep and res["dropped"] == ["t2"]
    ext, rec0, _ = _reconstruct(sq, world, world["ext"])
    con, rec1, _ = _reconstruct(sq, world, five)
    assert con["diagnostics"]["promoted"] == res["promoted"]
    print("promoted", res["promoted"])
    quant = sq.RTVQQuantizer(4, 2)
    for name in SHAPES:
        assert sorted(con["compressed"][name]) == keep
        total = {t: 0.0 for t in keep}
        for region, key in _regions(name):
            b1 = con["bases"][name][region]
            assert int(b1["N"]) == 5 and int(b1["k"]) + int(b1["U_low"].shape[1]) <= 4
            tag = f"{name} [{region}]"
            if tag in res["promoted"]:
                assert int(b1["U_low"].shape[1]) == 0 and res["promoted"][tag][1] == int(b1["k"]) > res["promoted"][tag][0]
            for t in keep:      # what is stored is finite, payload by payload
                a = con["compressed"][name][t][key]
                assert bool(torch.isfinite(a["c_high_fp16"].float()).all()), (tag, t)
                for pay in a["c_low_quant"]["payloads"]:
                    assert np.isfinite(float(pay["scale"])) and np.isfinite(float(pay["zero_point"])), (tag, t)
                if int(b1["U_low"].shape[1]):
                    assert bool(torch.isfinite(quant.dequantize(a["c_low_quant"], device="cpu")).all()), (tag, t)
            bounds, _ = _bound(sq, ext, con, con["diagnostics"], name, region, key, keep)
            for t in keep:
                total[t] += bounds[t]
        for t in keep:
            assert bool(torch.isfinite(rec1[t][name]).all()), (t, name)
            diff = float((rec1[t][name].double() - rec0[t][name].double()).norm())
            assert diff <= total[t], (t, name, diff, total[t])
    assert sorted(rec1) == keep
    back = str(tmp_path / "back")
    sq.add_tasks_to_artifacts(five, world["base"], {"t2": world["ckpt"]["t2"]}, masks=world["masks"], output_dir=back,
                              device="cuda", extend_basis=True)
    art, rec2, _ = _reconstruct(sq, world, back)
    assert sorted(rec2) == sorted(ALL)
    for name in SHAPES:
        x = (world["ckpt"]["t2"][name] - world["base"][name]).double()
        got = rec2["t2"][name].double().cpu()
        if name == MASKED:      # the noise region comes back shrunk: compare where the mask selects
            m = world["masks"][name].cpu()
            x, got = x[m], got[m]
        assert float((got - x).norm()) <= 0.5 * float(x.norm()), name      # the task is back, not just the mean
        for t in keep:
            assert torch.equal(rec2[t][name], rec1[t][name]), (t, name)      # nothing old moves (extend_basis' contract)


def _erase(tree, tasks):
    """A manifest key tree without shapes and with task names replaced, for comparing layouts of different stores."""
    if isinstance(tree, dict):
        if "tensor" in tree and "shape" in tree:
            return {"tensor": tree["tensor"], "device": tree["device"], "dims": len(tree["shape"])}
        if "torch.Size" in tree:
            return {"torch.Size": len(tree["torch.Size"])}
        return {("TASK" if k in tasks else k): _erase(v, tasks) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_erase(v, tasks) for v in tree]
    return tree


def test_a_reference_loader_could_read_it(sq, world):
    """File set and key trees of the consolidated store against tests/golden/artifact_manifest.json (written from the
    files the reference's own writer produced): the same files per parameter, the same trees per file kind."""
    meta = json.load(open(os.path.join(GOLDEN, "artifact_manifest.json")))
    gold = meta["manifest"]
    ours = artifact_manifest(world["con"])
    safe = {n: n.replace("/", "_") for n in SHAPES}
    assert sorted(ours) == sorted([f"basis/{s}.pt" for s in safe.values()] + [f"coeffs/{s}.pt" for s in safe.values()] +
                                  ["config.json", "diagnostics.json"])
    gtasks = {f"T{i}" for i in range(6)}
    g_basis = _erase(gold["basis/b.weight.pt"], gtasks)          # a parameter with a noise region
    g_plain = _erase(gold["basis/a.bias.pt"], gtasks)
    g_coef_t = _erase(gold["coeffs/b.weight.pt"], gtasks)["dict"]["TASK"]
    g_plain_t = _erase(gold["coeffs/a.bias.pt"], gtasks)["dict"]["TASK"]
    for name, s in safe.items():
        assert _erase(ours[f"basis/{s}.pt"], set(ALL)) == (g_basis if name == MASKED else g_plain), name
        tree = _erase(ours[f"coeffs/{s}.pt"], set(ALL))
        assert list(tree["dict"]) == ["TASK"]      # every task has the same tree
        assert tree["dict"]["TASK"] == (g_coef_t if name == MASKED else g_plain_t), name
    assert sorted(ours["config.json"]) == sorted(gold["config.json"]) == sorted(meta["config_fields"])


def test_against_the_materialising_route(sq, world):
    """The route there was before: reconstruct_task_vectors for all six tasks of the extended store (full-shape deltas;
    the masked parameter's noise region comes back times svd_noise_shrink), then run_basis_and_compress -- build_bases and
    compress_all_parameters -- on the results with the same config and masks.  Per region the same k, and sigma within
    the sum of both routes' resolutions; the materialising route's noise-region sigma is compared after dividing by the
    shrink it was reconstructed with.  Consolidation: eta / (1.866 sigma') (Weyl on K, the kept lambda above 4 eta) plus
    the fp32 rounding of sigma'.  The materialising route sees the fp32 results of the reconstruction (the (r + 3) 2^-24
    of its fma chains and one more rounding for the shrink: a perturbation of the stack of at most (r + 4) 2^-24
    || |A| |B| ||_F, which moves every singular value by at most that, Weyl) and resolves sigma to rtol 2e-5 of sigma_0
    (DESIGN.md section 2)."""
    art, rec, _ = _reconstruct(sq, world, world["ext"])
    cfg = art["config"]
    assert sorted(rec) == sorted(ALL)
    fresh, fcomp = sq.run_basis_and_compress({t: {n: rec[t][n].cuda() for n in SHAPES} for t in ALL}, world["masks"],
                                             cfg, "cuda")
    res = sq.consolidate_bases(art["compressed"], art["bases"], cfg, device="cuda")
    assert res["promoted"] == {}
    for name in SHAPES:
        assert sorted(fcomp[name]) == sorted(ALL)
        for region, key in _regions(name):
            b0, U0, m0, C0, _ = _region_arrays(sq, art, name, region, key, ALL)
            A = np.concatenate([U0, m0[:, None]], axis=1)
            B = np.stack([np.concatenate([C0[t], [1.0]]) for t in ALL], axis=1)
            shrink = float(cfg.svd_noise_shrink) if region == "noise" else 1.0
            bf, bc = fresh[name][region], res["bases"][name][region]
            s_f = bf["singular_values"].double().cpu().numpy() / shrink
            s_c = bc["singular_values"].double().cpu().numpy()
            r1 = s_c.size
            eta = res["noise_floor"][(name, region)]
            r = U0.shape[1]
            lim = eta / (1.866 * s_c) + 2.0 ** -23 * s_c + 2e-5 * s_f[0] + \
                (r + 4) * U32 * np.linalg.norm(np.abs(A) @ np.abs(B))
            print(name, region, "sigma consolidate", s_c, "materialised", s_f[:r1], "limit", lim)
            assert (np.abs(s_c - s_f[:r1]) <= lim).all(), (name, region)
            assert int(bc["k"]) == int(bf["k"]), (name, region, int(bc["k"]), int(bf["k"]))


def test_basis_report_of_the_consolidated_store(sq, world):
    """max |U'^T U' - I| per region through the existing basis_report (clustering.task_gram_from_artifacts on the adopted
    consolidated store).  Exactly, U' = A W has W^T (A^T A) W = I + Sigma^-1 V^T dK V Sigma^-1, every entry within
    eta / sigma_min^2; rounding U' to fp16 moves an entry by at most 2 * 2^-11 (1 + 2^-12) |u'_i| |u'_j| <= 1.1 * 2^-10 for
    column norms <= 1.05 (asserted through the limit itself); the rebase chain and the measuring Gram add less than
    2^-14 together (tests/test_hip_consolidate.py, test_designed_spectra)."""
    from svdq_amd.clustering import task_gram_from_artifacts
    art = sq.load_all_artifacts(world["con"])
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    G, tasks, report = task_gram_from_artifacts(ac, ab, device="cuda", basis_report=True)
    assert tasks == sorted(ALL) and np.isfinite(G).all()
    dg = art["diagnostics"]
    for name in SHAPES:
        for region, _ in _regions(name):
            tag = f"{name} [{region}]"
            sv = art["bases"][name][region]["singular_values"].double().numpy()
            lim = dg["noise_floor"][tag] / sv.min() ** 2 + 1.1 * 2.0 ** -10 + 2.0 ** -14
            print(tag, "max |U^T U - I|", report[tag], "limit", lim)
            assert lim < 0.1 and report[tag] <= lim, (tag, report[tag], lim)


def test_remerge_of_an_unmasked_store(sq, tmp_path):
    """remerge_from_artifacts takes no masks, so it is exact for unmasked stores only: an unmasked six-task store and its
    consolidation (to another threshold) are both merged again by it, and the two merged models agree within the weighted
    sum of the per-task bounds of the module docstring, plus the merge's own fma chains (the evaluation terms again) and
    the fp32 rounding of base + delta on either side (2^-24 of the merged model each)."""
    from oracle import svd_hybrid_oracle as orc
    shapes = {"u.a": (33, 21), "u.b": (515,)}
    g = torch.Generator().manual_seed(8)
    base = {n: torch.randn(s, generator=g) for n, s in shapes.items()}
    tv = {t: {} for t in ALL}
    for j, (n, s) in enumerate(shapes.items()):
        for t, d in zip(ALL, orc.synthetic_deltas(int(np.prod(s)), 6, 700 + j)):
            tv[t][n] = d.view(s).cuda()
    cfg = sq.SVDHybridConfig(tasks=list(ALL), svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4,
                             svd_rtvq_stages=2, svd_center=True)
    bases, comp = sq.run_basis_and_compress(tv, {}, cfg, "cuda")
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "con")
    diag = {"per_parameter": {n: {"original_shape": list(s)} for n, s in shapes.items()},
            "task_weights": {t: w for t, w in zip(ALL, (0.3, 0.1, 0.2, 0.1, 0.2, 0.1))}}
    sq.save_all_artifacts(bases, comp, diag, cfg, d0)
    res = sq.consolidate_artifacts(d0, output_dir=d1, energy_threshold=0.95)
    assert res["skipped"] == [] and sq.load_config(d1).svd_energy_threshold == 0.95
    m0 = sq.remerge_from_artifacts(d0, base, device="cuda")
    m1 = sq.remerge_from_artifacts(d1, base, device="cuda")
    assert m0["weights"] == m1["weights"] == diag["task_weights"]
    a0, a1 = sq.load_all_artifacts(d0), sq.load_all_artifacts(d1)
    for n in shapes:
        bounds, evs = _bound(sq, a0, a1, a1["diagnostics"], n, "masked", "masked", ALL)
        w = m1["weights"]
        x0, x1 = m0["merged_state_dict"][n].double().cpu(), m1["merged_state_dict"][n].double().cpu()
        lim = sum(w[t] * (bounds[t] + 2 * evs[t]) for t in ALL) + U32 * float(x0.norm() + x1.norm())
        diff = float((x1 - x0).norm())
        print(n, "merged models differ by", diff, "limit", lim)
        assert bool(torch.isfinite(x1).all()) and diff <= lim, (n, diff, lim)
