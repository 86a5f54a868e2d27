"""
CPU-only checks of the EMR merge (svdq_emr.hip and what is built on it): the four new entry points are declared,
exported and bound; bad arguments are refused before any device work, with an error text that names the entry point; the
Python surface has the signature the documents give and its refusals; the three files of a merge round-trip -- the mask
file through ``load_tall_mask_file`` -- on data made by tests/emr_model.py; the script's command line parses.
"""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import emr_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_emr_state_bytes", "svdq_emr_work_bytes", "svdq_plan_emr_elect", "svdq_emr_apply")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd


def test_new_entry_points_are_declared_exported_and_bound(sq):
    header = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sq._native.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T svdq_" in ln}
    lib = sq._native.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in sq._native.SIGNATURES and hasattr(lib, name)
    # the bindings against the declarations, argument by argument
    for name, count in (("svdq_plan_emr_elect", 15), ("svdq_emr_apply", 9)):
        decl = re.search(rf"int\s+{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        args = [" ".join(a.split()) for a in decl.split(",")]
        res, bound = sq._native.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(bound) == count, name
        for text, ctype in zip(args, bound):
            if "*" in text:
                assert ctype is ctypes.c_void_p, text
            else:
                assert ctype is {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[text.split()[0]], text
    decl = re.search(r"int\s+svdq_plan_emr_elect\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert [" ".join(a.split()).split()[-1].lstrip("*") for a in decl.split(",")][7:] == [
        "n_out", "n_tasks", "bit_base_dev", "uni_ptrs_dev", "mask_ptrs_dev", "state_dev", "work_dev", "stream"]
    assert sq._native.SIGNATURES["svdq_emr_state_bytes"] == (ctypes.c_int64, [ctypes.c_int32])
    assert sq._native.SIGNATURES["svdq_emr_work_bytes"] == (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int32,
                                                                             ctypes.c_int32])
    # the header states the definition, and which lines of it are decisions, next to the entry points
    doc = header[header.index("the EMR merge of a store"):header.index("int64_t svdq_emr_state_bytes")]
    for word in ("Huang et al. 2024", "S = S + v_g", "gamma = +1 if S > 0", "copysign(eps, gamma)", "DECISION",
                 "v_g * gamma > 0", "A_g = sum |v_g[d]|", "B_g = sum M_g[d] * eps[d]", "lambda_g = 1.0 when B_g == 0",
                 "lambda32 * (M_g[d] ? tau_uni[d] : +0)", "bit 7 - (i & 7) of byte i >> 3", "bit_base[p] + d",
                 "no floating-point", "ascending", "same bits on every call", "out may alias base"):
        assert word in doc, word
    assert doc.count("DECISION") >= 2
    # built like its siblings: no contraction of a product and a sum
    mk = open(os.path.join(os.path.dirname(sq._native.LIB_PATH), "csrc", "Makefile")).read()
    assert "build/svdq_emr.o" in mk and re.search(r"patsubst[^\n]*\bemr\b[^\n]*EXTRA := \$\(NOFMA\)", mk)


def test_bad_arguments_are_refused_before_any_launch(sq):
    lib, EINVAL, nat = sq._native.lib(), sq._native.SVDQ_EINVAL, sq._native
    assert lib.svdq_emr_state_bytes(0) == 0 and lib.svdq_emr_state_bytes(nat.MAX_TASKS + 1) == 0
    for T in (1, 8, 32):
        need = lib.svdq_emr_state_bytes(T)
        assert need % 256 == 0 and 0 <= need - 8 * 2 * T < 256
    assert lib.svdq_emr_work_bytes(None, 8, 8) == 0
    none = [None] * 7
    assert lib.svdq_plan_emr_elect(*none, 8, 8, None, None, None, None, None, None) == EINVAL
    assert "svdq_plan_emr_elect" in nat.last_error()
    # tables that are not NULL (never touched: the checks come first)
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    for n_out, T in ((0, 8), (8, 0), (nat.MAX_TASKS + 1, 8), (8, nat.MAX_TASKS + 1)):
        assert lib.svdq_plan_emr_elect(p, None, p, p, p, p, p, n_out, T, p, p, p, p, p, None) == EINVAL, (n_out, T)
        assert "svdq_plan_emr_elect" in nat.last_error() and "n_tasks" in nat.last_error()

    def apply(n=3, rows=p, bits=p, uni=p, stream=p, lam=1.0, outs=p):
        return lib.svdq_emr_apply(n, rows, bits, uni, stream, lam, None, outs, None)
    for kw, word in ((dict(rows=None), "rows"), (dict(bits=None), "bit_base"), (dict(uni=None), "uni_ptrs"),
                     (dict(stream=None), "mask_stream"), (dict(outs=None), "out_ptrs"), (dict(n=0), "n_params"),
                     (dict(n=-4), "n_params"), (dict(n=7680), "n_params"), (dict(lam=float("nan")), "lambda32"),
                     (dict(lam=float("inf")), "lambda32"), (dict(lam=float("-inf")), "lambda32")):
        assert apply(**kw) == EINVAL, kw
        assert "svdq_emr_apply" in nat.last_error() and word in nat.last_error(), (kw, nat.last_error())
    assert not buf.any()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.emr_merge_parameters) == [
        ("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E), ("tasks", None),
        ("reference_state_dict", None), ("remove_keys", None), ("device", "cuda"), ("return_stats", False)]
    assert sq.emr_merge_parameters is sq.merge.emr_merge_parameters
    assert params(sq.emr_task_state_dict) == [
        ("unified", E), ("masks", E), ("rescalers", E), ("task", E), ("base_state_dict", None),
        ("reference_state_dict", None), ("remove_keys", None), ("rescale", None), ("device", "cuda")]
    assert sq.emr_task_state_dict is sq.merge.emr_task_state_dict
    assert params(sq.emr_from_artifacts)[:3] == [("artifact_dir", E), ("output_dir", E), ("tasks", None)]
    assert params(sq.emr_task_model_from_files)[:4] == [("output_dir", E), ("task", E), ("base_model_path", E),
                                                        ("output_path", None)]
    assert sq.emr_from_artifacts is sq.storage.emr_from_artifacts
    assert callable(sq.CompressPlan.emr_elect)


def _fake():
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}
    return {"w": {"A": art, "B": art}}, {"w": {"masked": {}, "noise": None}}, {"w": torch.Size([16])}


def test_tasks_and_plain_dictionaries_are_refused(sq):
    comp, bases, shapes = _fake()
    cfg = sq.SVDHybridConfig()
    with pytest.raises(ValueError, match="unknown task 'Z'"):
        sq.emr_merge_parameters(comp, bases, shapes, cfg, tasks=["A", "Z"])
    with pytest.raises(ValueError, match="emr_merge_parameters: parameter 'w' is not backed by a plan.*the EMR merge"):
        sq.emr_merge_parameters(comp, bases, shapes, cfg)
    many = {"w": {f"t{i:02d}": comp["w"]["A"] for i in range(33)}}
    with pytest.raises(ValueError, match="between 1 and 32 tasks"):
        sq.emr_merge_parameters(many, bases, shapes, cfg)


def _model_made():
    """Three tasks over three parameters from a seed, task 'b' lacking one: what an EMR merge returns, made by the model."""
    rng = np.random.default_rng(11)
    shapes = {"enc.w": (9, 7), "enc/b": (13,), "head": (3, 5, 2)}
    names = sorted(shapes)
    sizes = {n: int(np.prod(shapes[n])) for n in names}
    tasks = ["a", "b", "c"]
    D = sum(sizes.values())
    v = rng.standard_normal((3, D)).astype(np.float32)
    has = np.ones((3, D), dtype=bool)
    has[1, sizes["enc.w"]:sizes["enc.w"] + sizes["enc/b"]] = False
    r = em.emr_merge(v, has)
    off = {n: sum(sizes[m] for m in names[:i]) for i, n in enumerate(names)}
    unified = {n: torch.from_numpy(r["tau"][off[n]:off[n] + sizes[n]].copy()).view(shapes[n]) for n in names}
    per_param = {n: r["masks"][:, off[n]:off[n] + sizes[n]] for n in names}
    streams = em.pack_streams(per_param, off, D)
    masks = {t: torch.from_numpy(streams[g].copy()) for g, t in enumerate(tasks)}
    rescalers = dict(zip(tasks, r["lambda"].tolist()))
    stats = {"abs_sum": dict(zip(tasks, r["A"].tolist())), "masked_sum": dict(zip(tasks, r["B"].tolist())),
             "active": dict(zip(tasks, r["masks"].sum(axis=1).tolist())), "rows": D}
    return shapes, names, sizes, tasks, unified, masks, rescalers, stats, per_param


def test_the_files_of_a_merge_round_trip(sq, tmp_path):
    shapes, names, sizes, tasks, unified, masks, rescalers, stats, per_param = _model_made()
    out = str(tmp_path / "emr")
    paths = sq.storage.save_emr_merge(out, unified, masks, rescalers, stats)
    assert sorted(os.listdir(out)) == ["EMR_mask_3task.npz", "emr_rescalers.json", "emr_unified.pt"]
    assert sorted(os.path.basename(p) for p in paths.values()) == sorted(os.listdir(out))
    # the mask file is a TALL mask container: the package's loader reads it with the unified tensors as the reference
    loaded = sq.load_tall_mask_file(paths["masks"], unified)
    assert sorted(loaded) == tasks
    for g, t in enumerate(tasks):
        for n in names:
            assert loaded[t][n].dtype is torch.bool and tuple(loaded[t][n].shape) == shapes[n]
            assert np.array_equal(loaded[t][n].numpy().reshape(-1), per_param[n][g]), (t, n)
    assert not loaded["b"]["enc/b"].any() and loaded["a"]["enc/b"].any()      # b lacks it
    record = json.load(open(paths["rescalers"]))
    assert record["tasks"] == tasks and record["mask_file"] == "EMR_mask_3task.npz" and record["rows"] == stats["rows"]
    assert record["rescalers"] == rescalers and record["abs_sum"] == stats["abs_sum"]      # floats read back exactly
    assert record["masked_sum"] == stats["masked_sum"] and record["active"] == stats["active"]
    u2, m2, r2, rec2 = sq.storage.load_emr_merge(out)
    assert rec2 == record and r2 == rescalers and sorted(u2) == names and sorted(m2) == tasks
    for n in names:
        assert u2[n].shape == unified[n].shape and torch.equal(u2[n].view(torch.int32), unified[n].view(torch.int32))
    for t in tasks:
        assert m2[t].dtype is torch.uint8 and torch.equal(m2[t], masks[t])
    assert not (len(set(rescalers.values())) == 1)


def test_task_state_dict_refusals_come_before_device_work(sq, tmp_path):
    shapes, names, sizes, tasks, unified, masks, rescalers, stats, _ = _model_made()
    who = "emr_task_state_dict"
    with pytest.raises(ValueError, match=f"{who}: unknown task 'z'"):
        sq.emr_task_state_dict(unified, masks, rescalers, "z")
    for bad in (float("nan"), float("inf"), 1e39, "1.0", True):
        with pytest.raises(ValueError, match=f"{who}: the rescaler of task 'a'"):
            sq.emr_task_state_dict(unified, masks, rescalers, "a", rescale=bad)
    with pytest.raises(ValueError, match=f"{who}: the rescaler of task 'a' is missing"):
        sq.emr_task_state_dict(unified, masks, {"b": 1.0}, "a")
    with pytest.raises(ValueError, match=f"{who}: the mask of task 'a' must be a uint8 tensor of 14 bytes"):
        sq.emr_task_state_dict(unified, dict(masks, a=masks["a"][:-1]), rescalers, "a")
    with pytest.raises(ValueError, match=f"{who}: parameter 'head' of the store has no place in the mask streams"):
        sq.emr_task_state_dict(unified, masks, rescalers, "a", remove_keys=["head"])
    ref = {n: torch.empty(sizes[n] + (n == "head"), device="meta") for n in names}
    with pytest.raises(ValueError, match=rf"{who}: reference_state_dict\['head'\] has 31 elements, the store holds 30"):
        sq.emr_task_state_dict(unified, masks, rescalers, "a", reference_state_dict=ref)
    with pytest.raises(ValueError, match="unknown task 'z'"):
        sq.storage.save_emr_merge(str(tmp_path), unified, masks, rescalers, stats)
        sq.storage.emr_task_model_from_files(str(tmp_path), "z", {})


def test_script_help_parses():
    script = os.path.join(ROOT, "scripts", "emr_merge.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--output-dir", "--tasks", "--task", "--base-model-path", "--output-path"):
        assert flag in r.stdout
    r = subprocess.run([sys.executable, script, "--output-dir", "/nonexistent"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--artifact-dir" in r.stderr
