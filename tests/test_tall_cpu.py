"""
CPU-only checks of the TALL masks and the consensus merge (svdq_tall.hip and what is built on it): the two new entry
points are declared, exported and bound; bad arguments are refused before any device work, with an error text that names
the entry point; the Python surface has the signature the documents give and its refusals; the script's command line
parses.
"""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_tall_work_bytes", "svdq_plan_tall_consensus")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd


def test_new_entry_points_are_declared_exported_and_bound(sq):
    import ctypes
    header = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sq._native.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T svdq_" in ln}
    lib = sq._native.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in sq._native.SIGNATURES and hasattr(lib, name)
    # the binding against the declaration, argument by argument
    decl = re.search(r"int\s+svdq_plan_tall_consensus\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    res, bound = sq._native.SIGNATURES["svdq_plan_tall_consensus"]
    assert res is ctypes.c_int32 and len(args) == len(bound) == 19
    for text, ctype in zip(args, bound):
        if "*" in text:
            assert ctype is ctypes.c_void_p, text
        else:
            want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[text.split()[0]]
            assert ctype is want, text
    assert [a.split()[-1].lstrip("*") for a in args][7:19] == [
        "n_out", "n_tasks", "bit_base_dev", "lambdas_dev", "min_agree", "scaling", "base_ptrs_dev", "out_ptrs_dev",
        "mask_ptrs_dev", "state_dev", "work_dev", "stream"]
    assert sq._native.SIGNATURES["svdq_tall_work_bytes"] == (ctypes.c_int64, [ctypes.c_int32])
    # the header states the definition next to the entry points
    doc = header[header.index("TALL masks and the consensus merge of a store"):header.index("int64_t svdq_tall_work_bytes")]
    for word in ("Wang et al. 2024", "S = S + v_g", "R_g = S - v_g", "|v_g| > lambda_g * |R_g|", "STRICT", 'writes ">="',
                 "c >= min_agree", "kept ? S : +0", "numpy.packbits", "bit 7 - (i & 7) of", "byte i >> 3",
                 "bit_base[p] + d", "active [T]", "agree [T + 1]", "two calls give identical bits"):
        assert word in doc, word
    # built like svdq_ties.hip and svdq_dare.hip: no contraction of a product and a sum
    mk = open(os.path.join(os.path.dirname(sq._native.LIB_PATH), "csrc", "Makefile")).read()
    assert "build/svdq_tall.o" in mk and re.search(r"patsubst[^\n]*\btall\b[^\n]*EXTRA := \$\(NOFMA\)", mk)


def test_bad_arguments_are_refused_before_any_launch(sq):
    lib, EINVAL = sq._native.lib(), sq._native.SVDQ_EINVAL
    assert lib.svdq_tall_work_bytes(0) == 0 and lib.svdq_tall_work_bytes(sq._native.MAX_TASKS + 1) == 0
    for T in (1, 8, 32):
        need = lib.svdq_tall_work_bytes(T)
        assert need % 256 == 0 and 0 <= need - 8 * (2 * T + 1) < 256
    none = [None] * 7
    assert lib.svdq_plan_tall_consensus(*none, 8, 8, None, None, 2, 1.0, None, None, None, None, None, None) == EINVAL
    assert "svdq_plan_tall_consensus" in sq._native.last_error()
    # tables that are not NULL (never touched: the checks come first)
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()

    def call(n_out=8, T=8, bit_base=p, lambdas=p, k=2, outs=p, masks=p):
        return lib.svdq_plan_tall_consensus(p, None, p, p, p, p, p, n_out, T, bit_base, lambdas, k, 1.0, None, outs, masks,
                                            p, p, None)
    for n_out, T in ((0, 8), (8, 0), (sq._native.MAX_TASKS + 1, 8), (8, sq._native.MAX_TASKS + 1)):
        assert call(n_out=n_out, T=T) == EINVAL, (n_out, T)
        assert "svdq_plan_tall_consensus" in sq._native.last_error() and "n_tasks" in sq._native.last_error()
    assert not buf.any()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.consensus_merge_parameters) == [
        ("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E), ("tall_lambda", 0.4), ("k", 2),
        ("scaling", 1.0), ("tasks", None), ("base_state_dict", None), ("reference_state_dict", None),
        ("remove_keys", None), ("return_masks", False), ("device", "cuda"), ("return_stats", False)]
    assert sq.consensus_merge_parameters is sq.merge.consensus_merge_parameters
    assert params(sq.tall_masks_from_store) == [
        ("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E), ("tall_lambda", 0.4), ("tasks", None),
        ("reference_state_dict", None), ("remove_keys", None), ("device", "cuda"), ("return_stats", False)]
    assert sq.tall_masks_from_store is sq.merge.tall_masks_from_store
    assert params(sq.consensus_merge_from_artifacts)[:4] == [("artifact_dir", E), ("base_model_path", E),
                                                             ("output_path", None), ("mask_output_path", None)]
    assert [n for n, _ in params(sq.consensus_merge_from_artifacts)[4:]] == ["tall_lambda", "k", "scaling", "tasks",
                                                                             "remove_keys", "device"]
    assert sq.consensus_merge_from_artifacts is sq.storage.consensus_merge_from_artifacts
    assert callable(sq.CompressPlan.tall_consensus)


def _fake():
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}
    return {"w": {"A": art, "B": art}}, {"w": {"masked": {}, "noise": None}}, {"w": torch.Size([16])}


@pytest.mark.parametrize("lam", [-0.1, float("nan"), float("inf"), None, "0.4", True, 1e39, {"A": 0.4},
                                 {"A": 0.4, "B": -1.0}, {"A": 0.4, "B": float("nan")}])
def test_a_lambda_outside_the_definition_is_a_value_error(sq, lam):
    comp, bases, shapes = _fake()
    cfg = sq.SVDHybridConfig()
    with pytest.raises(ValueError, match="tall_lambda"):      # before anything is looked at, also where no GPU is visible
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=lam)
    with pytest.raises(ValueError, match="tall_lambda"):
        sq.tall_masks_from_store(comp, bases, shapes, cfg, tall_lambda=lam)
    if not isinstance(lam, dict):
        with pytest.raises(ValueError, match="tall_lambda"):
            sq.consensus_merge_from_artifacts("/nonexistent", {}, tall_lambda=lam)


@pytest.mark.parametrize("k", [-1, 3, 2.0, None, "2", True])
def test_k_is_not_clamped(sq, k):
    comp, bases, shapes = _fake()      # two tasks: k = 3 is past them
    with pytest.raises(ValueError, match="k must be an integer"):
        sq.consensus_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig(), k=k)
    if k != 3:      # the task count is the store's to say
        with pytest.raises(ValueError, match="k must be an integer"):
            sq.consensus_merge_from_artifacts("/nonexistent", {}, k=k)


def test_tasks_and_plain_dictionaries_are_refused(sq):
    comp, bases, shapes = _fake()
    cfg = sq.SVDHybridConfig()
    with pytest.raises(ValueError, match="unknown task 'Z'"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tasks=["A", "Z"])
    with pytest.raises(ValueError, match="k must be an integer in \\[0, 1\\]"):      # k counts the MERGED tasks
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tasks=["A"], k=2)
    # the parameter is named, under this function's name; k = T, lambda 0 and per-task lambdas pass the argument checks
    with pytest.raises(ValueError,
                       match="consensus_merge_parameters: parameter 'w' is not backed by a plan.*the consensus merge"):
        sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda={"A": 0, "B": 2.5}, k=2)
    with pytest.raises(ValueError, match="tall_masks_from_store: parameter 'w' is not backed by a plan.*the TALL mask"):
        sq.tall_masks_from_store(comp, bases, shapes, cfg, tall_lambda=0.0)
    with pytest.raises(ValueError, match="ties_merge_parameters: parameter 'w' is not backed by a plan.*the TIES merge"):
        sq.ties_merge_parameters(comp, bases, shapes, cfg)


def test_script_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "consensus_merge.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--output-path", "--mask-output", "--tall-lambda", "--k",
                 "--scaling", "--tasks"):
        assert flag in r.stdout
