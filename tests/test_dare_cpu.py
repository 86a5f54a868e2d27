"""
CPU-only checks of the DARE merge (svdq_dare.hip and what is built on it): the two new entry points are declared,
exported and bound; bad arguments are refused before any device work, with an error text that names the entry point; the
Python surface has the signature the documents give and its refusals; the script's command line parses.
"""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_dare_work_bytes", "svdq_plan_dare_merge")


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
    decl = re.search(r"int\s+svdq_plan_dare_merge\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    res, bound = sq._native.SIGNATURES["svdq_plan_dare_merge"]
    assert res is ctypes.c_int32 and len(args) == len(bound) == 20
    for text, ctype in zip(args, bound):
        if "*" in text:
            assert ctype is ctypes.c_void_p, text
        else:
            want = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
                    "float": ctypes.c_float}[text.split()[0]]
            assert ctype is want, text
    assert [a.split()[-1].lstrip("*") for a in args][9:15] == ["row_base_dev", "weights_dev", "seed", "drop_threshold",
                                                               "keep_scale", "scaling"]
    assert sq._native.SIGNATURES["svdq_dare_work_bytes"] == (ctypes.c_int64, [ctypes.c_int32])
    # the header states the definition next to the entry points
    doc = header[header.index("drop-and-rescale (DARE) merge"):header.index("int64_t svdq_dare_work_bytes")]
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "g >> 2", "g & 3",
                 "word < drop_threshold", "task_arithmetic", "implements neither", "merge.py:144-194", "rtvq.py:85-103"):
        assert word in doc, word


def test_bad_arguments_are_refused_before_any_launch(sq):
    lib, EINVAL = sq._native.lib(), sq._native.SVDQ_EINVAL
    assert lib.svdq_dare_work_bytes(0) == 0 and lib.svdq_dare_work_bytes(sq._native.MAX_TASKS + 1) == 0
    for T in (1, 8, 32):
        need = lib.svdq_dare_work_bytes(T)
        assert need % 256 == 0 and 0 <= need - 8 * T < 256
    none = [None] * 7
    assert lib.svdq_plan_dare_merge(*none, 8, 8, None, None, 0, 0, 0.0, 1.0, None, None, None, None, None) == EINVAL
    assert "svdq_plan_dare_merge" in sq._native.last_error()
    # tables that are not NULL (never touched: the checks come first) and a task count out of range
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    for n_out, T in ((0, 8), (8, 0), (sq._native.MAX_TASKS + 1, 8), (8, sq._native.MAX_TASKS + 1)):
        assert lib.svdq_plan_dare_merge(p, None, p, p, p, p, p, n_out, T, p, p, 0, 0, 0.0, 1.0, None, p, p, p,
                                        None) == EINVAL, (n_out, T)
        assert "svdq_plan_dare_merge" in sq._native.last_error() and "n_tasks" in sq._native.last_error()
    assert not buf.any()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.dare_merge_parameters) == [("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E),
                                                ("drop_rate", 0.9), ("seed", 0), ("rescale", True), ("weights", None),
                                                ("normalize", False), ("scaling", 1.0), ("tasks", None),
                                                ("base_state_dict", None), ("device", "cuda"), ("return_stats", False)]
    assert sq.dare_merge_parameters is sq.merge.dare_merge_parameters
    assert params(sq.dare_merge_from_artifacts)[:4] == [("artifact_dir", E), ("base_model_path", E), ("output_path", None),
                                                        ("drop_rate", 0.9)]
    assert [n for n, _ in params(sq.dare_merge_from_artifacts)[4:]] == ["seed", "rescale", "weights", "normalize",
                                                                        "scaling", "tasks", "device"]
    assert sq.dare_merge_from_artifacts is sq.storage.dare_merge_from_artifacts
    assert callable(sq.CompressPlan.dare_merge)
    # _ties_jobs names its caller; the default keeps the TIES messages
    sig = inspect.signature(sq.merge._ties_jobs).parameters
    assert sig["who"].default == "ties_merge_parameters"


def _fake():
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}
    return {"w": {"A": art, "B": art}}, {"w": {"masked": {}, "noise": None}}, {"w": torch.Size([16])}


@pytest.mark.parametrize("drop_rate", [1.0, -0.1, 1.5, float("nan"), float("inf"), None, "0.5", True])
def test_drop_rate_outside_the_definition_is_a_value_error(sq, drop_rate):
    comp, bases, shapes = _fake()
    with pytest.raises(ValueError, match="drop_rate"):      # before anything is looked at, also where no GPU is visible
        sq.dare_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig(), drop_rate=drop_rate)
    with pytest.raises(ValueError, match="drop_rate"):
        sq.dare_merge_from_artifacts("/nonexistent", {}, drop_rate=drop_rate)


@pytest.mark.parametrize("seed", [-1, 1 << 64, 0.5, None, "7"])
def test_seed_outside_the_definition_is_a_value_error(sq, seed):
    comp, bases, shapes = _fake()
    with pytest.raises(ValueError, match="seed"):
        sq.dare_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig(), seed=seed)
    with pytest.raises(ValueError, match="seed"):
        sq.dare_merge_from_artifacts("/nonexistent", {}, seed=seed)


def test_weights_tasks_and_plain_dictionaries_are_refused(sq):
    comp, bases, shapes = _fake()
    cfg = sq.SVDHybridConfig()
    with pytest.raises(ValueError, match="weight of task 'B' is missing"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, weights={"A": 1.0})
    for bad in (float("nan"), float("inf"), None, "1", 1e39):      # 1e39 is not finite in fp32
        with pytest.raises(ValueError, match="weight"):
            sq.dare_merge_parameters(comp, bases, shapes, cfg, weights={"A": 1.0, "B": bad})
    with pytest.raises(ValueError, match="weights"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="non-zero sum"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, weights={"A": 1.0, "B": -1.0}, normalize=True)
    with pytest.raises(ValueError, match="unknown task 'Z'"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, tasks=["A", "Z"])
    # the parameter is named, under this function's name; the largest seed and drop rate 0 pass the argument checks
    with pytest.raises(ValueError, match="dare_merge_parameters: parameter 'w' is not backed by a plan.*the DARE merge"):
        sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.0, seed=(1 << 64) - 1, weights={"A": 2, "B": 0.5})
    with pytest.raises(ValueError, match="ties_merge_parameters: parameter 'w' is not backed by a plan.*the TIES merge"):
        sq.ties_merge_parameters(comp, bases, shapes, cfg)


def test_script_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "dare_merge.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--output-path", "--drop-rate", "--seed", "--no-rescale",
                 "--weights", "--normalize", "--scaling", "--tasks"):
        assert flag in r.stdout
