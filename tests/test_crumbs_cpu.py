"""
CPU-only checks of the Model Breadcrumbs merge (svdq_crumbs.hip and what is built on it): the new entry points are
declared, exported and bound; the header states the definition; bad arguments are refused before any device work, with
an error text that names the entry point; the Python surface has the signature the documents give; the script's command
line parses; the new object is compiled without fused multiply-adds.
"""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"svdq_crumbs_work_bytes": 2, "svdq_plan_crumbs_hist": 14, "svdq_plan_crumbs_select_step": 6,
       "svdq_plan_crumbs_merge": 17}


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
    for name, argc in NEW.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", code)
        assert decl, name
        assert len(decl.group(1).split(",")) == argc, name      # the declaration's argument count
        assert name in exported and name in sq._native.SIGNATURES and hasattr(lib, name)
        assert len(sq._native.SIGNATURES[name][1]) == argc, name
    assert re.search(r"#define\s+SVDQ_CRUMBS_DIGITS\s+4\b", code) and sq.pipeline.CRUMBS_DIGITS == 4


def test_the_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "svdq.h")).read()
    doc = header[header.index("Model Breadcrumbs merge of a store"):header.index("int64_t svdq_crumbs_work_bytes")]
    for word in ("Davari", "n_keep = int(D_p * density)", "n_top = int(D_p *", "n_bot = D_p - n_keep - n_top",
                 "n_top += n_bot", "(n_bot + 1)-th smallest", "(D_p - n_top)-th smallest", "lo <= m <= hi",
                 "kept >= n_keep", "no implicit zeros", "s == 0", "a / max(c, 1)", "base + scaling * merged",
                 "bounds 3", "2^32", "rtvq.py:85-103", "merge.py:144-194"):
        assert word in doc, word


def test_bad_arguments_are_refused_before_any_launch(sq):
    lib, EINVAL = sq._native.lib(), sq._native.SVDQ_EINVAL
    MAXT = sq._native.MAX_TASKS
    for P, T in ((0, 8), (-1, 8), (4, 0), (4, MAXT + 1)):
        assert lib.svdq_crumbs_work_bytes(P, T) == 0, (P, T)
    for P, T in ((1, 1), (7, 8), (300, 20), (11, 32)):
        need = lib.svdq_crumbs_work_bytes(P, T)
        # hist uint32 [P][2][T][256] | prefix, rank [P][2][T] | kept [P][T] | two counters (uint64 words)
        assert need % 256 == 0 and 0 <= need - 8 * (261 * P * T + 2) < 256, (P, T)
    assert lib.svdq_plan_crumbs_hist(None, None, None, None, None, None, None, 8, 8, 0, 3, None, None, None) == EINVAL
    assert "svdq_plan_crumbs_hist" in sq._native.last_error()
    assert lib.svdq_plan_crumbs_merge(None, None, None, None, None, None, None, 8, 8, 0, 0, 1.0, None, None, None, None,
                                      None) == EINVAL
    assert "svdq_plan_crumbs_merge" in sq._native.last_error()
    assert lib.svdq_plan_crumbs_select_step(None, 8, 0, None, None, None) == EINVAL
    assert "svdq_plan_crumbs_select_step" in sq._native.last_error()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.breadcrumbs_merge_parameters) == [
        ("compressed_all", E), ("bases", E), ("original_shapes", E), ("config", E), ("density", 0.9), ("gamma", 0.01),
        ("scaling", 1.0), ("sign_election", False), ("merge_func", "sum"), ("tasks", None), ("base_state_dict", None),
        ("device", "cuda"), ("return_stats", False)]
    assert sq.breadcrumbs_merge_parameters is sq.merge.breadcrumbs_merge_parameters
    assert params(sq.breadcrumbs_merge_from_artifacts) == [
        ("artifact_dir", E), ("base_model_path", E), ("output_path", None), ("density", 0.9), ("gamma", 0.01),
        ("scaling", 1.0), ("sign_election", False), ("merge_func", "sum"), ("tasks", None), ("device", "cuda")]
    assert sq.breadcrumbs_merge_from_artifacts is sq.storage.breadcrumbs_merge_from_artifacts
    for name in ("crumbs_hist", "crumbs_select", "crumbs_merge"):
        assert callable(getattr(sq.CompressPlan, name))
    assert sq.crumbs_thresholds is sq.pipeline.crumbs_thresholds and sq.CrumbsState is sq.pipeline.CrumbsState


def test_the_ranks_are_python_integers(sq):
    ranks = sq.merge.crumbs_ranks
    assert ranks(10, 0.5, 0.2) == (4, 8)       # n_keep 5, n_top 2, n_bot 3
    assert ranks(10, 0.5, 0.7) == (1, 5)       # n_bot -2: n_top gives way
    assert ranks(10, 1.0, 0.3) == (1, 10)      # density 1 keeps everything
    assert ranks(4, 0.2, 0.0) == (0, 0)        # n_keep 0
    assert ranks(1, 1.0, 0.5) == (1, 1)
    assert ranks(70001, 2 / 70001, 0.01) == (70001 - 2 - 700 + 1, 70001 - 700)


ART = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16)}}


def _call(sq, **kw):
    return sq.breadcrumbs_merge_parameters({"w": {"A": ART}}, {"w": {"masked": {}, "noise": None}},
                                           {"w": torch.Size([16])}, sq.SVDHybridConfig(), **kw)


@pytest.mark.parametrize("density", [0.0, -0.1, 1.5, float("nan"), None, True])
def test_density_outside_the_definition_is_a_value_error(sq, density):
    with pytest.raises(ValueError, match="density"):      # before anything is looked at, also where no GPU is visible
        _call(sq, density=density)
    with pytest.raises(ValueError, match="density"):
        sq.breadcrumbs_merge_from_artifacts("/nonexistent", {}, density=density)


@pytest.mark.parametrize("gamma", [-0.01, 1.0, 2.0, float("nan"), None])
def test_gamma_outside_the_definition_is_a_value_error(sq, gamma):
    with pytest.raises(ValueError, match="gamma"):
        _call(sq, gamma=gamma)
    with pytest.raises(ValueError, match="gamma"):
        sq.breadcrumbs_merge_from_artifacts("/nonexistent", {}, gamma=gamma)


@pytest.mark.parametrize("scaling", [float("inf"), float("nan"), None])
def test_a_scaling_that_is_not_finite_is_a_value_error(sq, scaling):
    with pytest.raises(ValueError, match="scaling"):
        _call(sq, scaling=scaling)


def test_merge_func_unknown_task_and_plain_dictionaries_are_refused(sq):
    with pytest.raises(ValueError, match="merge_func"):
        _call(sq, merge_func="median")
    with pytest.raises(ValueError, match="unknown task 'Z'"):
        _call(sq, tasks=["A", "Z"])
    with pytest.raises(ValueError, match="breadcrumbs_merge_parameters: parameter 'w' is not backed by a plan"):
        _call(sq)


def test_script_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "breadcrumbs_merge.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--density", "--gamma", "--scaling", "--sign-election",
                 "--merge-func", "--tasks", "--output-path"):
        assert flag in r.stdout


def test_the_new_object_is_compiled_without_fused_multiply_adds():
    mk = open(os.path.join(ROOT, "svd-quantization-task-merging_amd", "csrc", "Makefile")).read()
    rule = re.search(r"\$\(patsubst %,build/svdq_%\.o,([^)]*)\): EXTRA := \$\(NOFMA\)", mk)
    assert rule and "crumbs" in rule.group(1).split() and "ties" in rule.group(1).split()
    assert "build/svdq_crumbs.o" in re.search(r"^OBJS\s*:=(.*)$", mk, flags=re.M).group(1).split()
