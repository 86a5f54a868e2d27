"""
CPU-only checks of the TIES merge (svdq_ties.hip and what is built on it): the new entry points are declared, exported
and bound; bad arguments are refused before any device work, with an error text that names the entry point; the Python
surface has the signature the documents give; the script's command line parses.
"""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_ties_work_bytes", "svdq_plan_ties_hist", "svdq_ties_select_step", "svdq_plan_ties_merge")


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
    assert len(sq._native.SIGNATURES["svdq_plan_ties_hist"][1]) == 13
    assert len(sq._native.SIGNATURES["svdq_plan_ties_merge"][1]) == 16
    assert re.search(r"#define\s+SVDQ_TIES_DIGITS\s+4\b", code) and sq.pipeline.TIES_DIGITS == 4
    # the header states the definition next to the entry points
    doc = header[header.index("sign-elected (TIES) merge"):header.index("int64_t svdq_ties_work_bytes")]
    for word in ("trim", "elect", "s == 0", "merge.py:144-194", "rtvq.py:85-103"):
        assert word in doc, word


def test_bad_arguments_are_refused_before_any_launch(sq):
    lib, EINVAL = sq._native.lib(), sq._native.SVDQ_EINVAL
    # the state table: hist [T][256] | prefix | rank | kept | two counters, in uint64 words, rounded up to 256 bytes
    assert lib.svdq_ties_work_bytes(0) == 0 and lib.svdq_ties_work_bytes(sq._native.MAX_TASKS + 1) == 0
    for T in (1, 8, 32):
        need = lib.svdq_ties_work_bytes(T)
        assert need % 256 == 0 and 0 <= need - 8 * (259 * T + 2) < 256
    assert lib.svdq_plan_ties_hist(None, None, None, None, None, None, None, 8, 8, 0, None, None, None) == EINVAL
    assert "svdq_plan_ties_hist" in sq._native.last_error()
    assert lib.svdq_plan_ties_merge(None, None, None, None, None, None, None, 8, 8, 0, 1.0, None, None, None, None,
                                    None) == EINVAL
    assert "svdq_plan_ties_merge" in sq._native.last_error()
    assert lib.svdq_ties_select_step(None, 8, 0, 1, None, None) == EINVAL
    assert "svdq_ties_select_step" in sq._native.last_error()
    # a table that is not NULL (never touched: the checks come first), a task count or a digit out of range
    buf = torch.zeros(8 * (259 * 32 + 2) + 256, dtype=torch.uint8)
    for T, digit, rank in ((0, 0, 1), (sq._native.MAX_TASKS + 1, 0, 1), (8, -1, 1), (8, 4, 1), (8, 0, 0)):
        assert lib.svdq_ties_select_step(buf.data_ptr(), T, digit, rank, None, None) == EINVAL, (T, digit, rank)
        assert "svdq_ties_select_step" in sq._native.last_error()
    assert not buf.any()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.ties_merge_parameters) == [("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E),
                                                ("density", 0.2), ("scaling", 1.0), ("merge_func", "mean"),
                                                ("tasks", None), ("base_state_dict", None), ("device", "cuda"),
                                                ("return_stats", False)]
    assert sq.ties_merge_parameters is sq.merge.ties_merge_parameters
    assert params(sq.ties_merge_from_artifacts) == [("artifact_dir", E), ("base_model_path", E), ("output_path", None),
                                                    ("density", 0.2), ("scaling", 1.0), ("merge_func", "mean"),
                                                    ("tasks", None), ("device", "cuda")]
    assert sq.ties_merge_from_artifacts is sq.storage.ties_merge_from_artifacts
    assert callable(sq.CompressPlan.ties_hist) and callable(sq.CompressPlan.ties_merge)
    assert sq.ties_thresholds is sq.pipeline.ties_thresholds


@pytest.mark.parametrize("density", [0.0, -0.1, 1.5, float("nan"), None])
def test_density_outside_the_definition_is_a_value_error(sq, density):
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}
    with pytest.raises(ValueError, match="density"):      # before anything is looked at, also where no GPU is visible
        sq.ties_merge_parameters({"w": {"A": art}}, {"w": {"masked": {}}}, {"w": torch.Size([16])}, sq.SVDHybridConfig(),
                                 density=density)
    with pytest.raises(ValueError, match="density"):
        sq.ties_merge_from_artifacts("/nonexistent", {}, density=density)


def test_merge_func_and_plain_dictionaries_are_refused(sq):
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}
    comp, bases, shapes = {"w": {"A": art}}, {"w": {"masked": {}, "noise": None}}, {"w": torch.Size([16])}
    with pytest.raises(ValueError, match="merge_func"):
        sq.ties_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig(), merge_func="median")
    with pytest.raises(ValueError, match="unknown task 'Z'"):
        sq.ties_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig(), tasks=["A", "Z"])
    with pytest.raises(ValueError, match="'w' is not backed by a plan"):      # the parameter is named
        sq.ties_merge_parameters(comp, bases, shapes, sq.SVDHybridConfig())


def test_script_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ties_merge.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--output-path", "--density", "--scaling", "--merge-func",
                 "--tasks"):
        assert flag in r.stdout
