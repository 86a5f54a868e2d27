"""
Host side of the store Gram, without a GPU: the two entry points are declared, exported and bound; the Python
signatures; a numpy model of the host scatter (per-parameter matrices with differing task lists -> the sorted-task
N x N matrix, against a dense fp64 Gram of zero-filled vectors); the ValueError on a non-finite matrix; the loud failure
without a GPU; scripts/remerge.py --help.
"""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_plan_store_gram", "svdq_plan_store_gram_work_bytes")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd


def test_symbols_declared_exported_and_bound(sq):
    from ctypes import c_int32, c_int64, c_void_p
    text = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sq._native.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T svdq_" in ln}
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in exported and name in sq._native.SIGNATURES
        assert hasattr(sq._native.lib(), name)
    assert sq._native.SIGNATURES["svdq_plan_store_gram_work_bytes"] == (c_int64, [c_void_p])
    assert sq._native.SIGNATURES["svdq_plan_store_gram"] == (c_int32, [c_void_p] * 9)
    # the contract is stated once, at the declaration, and cites the reference lines it replaces
    doc = text[text.index("the task Gram of a STORE"):text.index("int64_t svdq_plan_store_gram_work_bytes")]
    assert "clustering.py:55-120" in doc and "clustering.py:198-245" in doc
    assert sq._native.lib().svdq_abi_version() == 1
    # a translation unit of its own, compiled like the other consumers
    mk = open(os.path.join(ROOT, "svd-quantization-task-merging_amd", "csrc", "Makefile")).read()
    assert "build/svdq_store_gram.o" in mk
    profile = open(os.path.join(ROOT, "profiles", "store_gram_resource_usage.txt")).read()
    assert profile.count("k_store_gram") >= 7 and "ScratchSize [bytes/lane]: 0" in profile
    assert not re.search(r"ScratchSize \[bytes/lane\]: [1-9]", profile)


def test_python_signatures(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.CompressPlan.store_gram) == [("self", E), ("rows_dev", None), ("basis_gram", False)]
    assert params(sq.task_gram_from_artifacts) == [("compressed_all", E), ("bases", E), ("device", "cuda"),
                                                   ("basis_report", False)]
    assert params(sq.cluster_tasks_from_artifacts) == [("compressed_all", E), ("bases", E), ("k", E),
                                                       ("method", "kmeans"), ("device", "cuda")]
    assert params(sq.remerge_from_artifacts) == [("artifact_dir", E), ("base_model_path", E), ("output_path", None),
                                                 ("weighting", None), ("cluster_k", None), ("performance_file", None),
                                                 ("temperature", None), ("device", "cuda"), ("update_store", False)]
    # the functions beside them keep theirs
    assert params(sq.add_tasks_to_artifacts)[:4] == [("artifact_dir", E), ("base_state_dict", E), ("finetuned", E),
                                                     ("masks", None)]
    assert params(sq.reconstruct_from_artifacts) == [("artifact_dir", E), ("base_model_path", E), ("output_path", None),
                                                     ("device", "cpu")]


def _model(rng):
    """Three parameters over tasks a..d: who holds which, in which plan order, and the vectors themselves."""
    tasks = ["a", "b", "c", "d"]
    layout = {"w.2": (["d", "a", "c", "b"], 5), "w.0": (["c", "a"], 7), "w.1": (["b", "d", "a"], 3)}
    vec = {n: {t: rng.standard_normal(D) for t in order} for n, (order, D) in layout.items()}
    return tasks, layout, vec


def test_assemble_matches_the_dense_gram_of_zero_filled_vectors(sq):
    rng = np.random.default_rng(3)
    tasks, layout, vec = _model(rng)
    per_param = {}
    for n, (order, D) in layout.items():
        X = np.stack([vec[n][t] for t in order])
        if n == "w.2":      # a parameter in two pieces (signal and noise rows of a masked entry): disjoint rows
            per_param[n] = [(X[:, :2] @ X[:, :2].T, order), (X[:, 2:] @ X[:, 2:].T, order)]
        else:
            per_param[n] = [(X @ X.T, order)]
    G = sq.assemble_task_gram(per_param, tasks)
    # flatten_task_vectors: parameters in sorted order, zeros where a task lacks one
    full = np.concatenate([np.stack([vec[n].get(t, np.zeros(layout[n][1])) for t in tasks]) for n in sorted(layout)],
                          axis=1)
    assert full.shape == (4, 15)
    np.testing.assert_allclose(G, full @ full.T, rtol=0, atol=1e-13)
    assert np.array_equal(G, G.T)
    # "b" lacks w.0: its row holds w.1 and w.2 alone
    i = tasks.index("b")
    want = sum(np.array([vec[n]["b"] @ vec[n].get(t, np.zeros(layout[n][1])) for t in tasks]) for n in ("w.1", "w.2"))
    np.testing.assert_allclose(G[i], want, rtol=0, atol=1e-13)
    # the order of the dictionary does not enter: parameters are added in sorted-name order
    again = sq.assemble_task_gram(dict(reversed(list(per_param.items()))), tasks)
    assert np.array_equal(G, again)
    assert not sq.assemble_task_gram({}, tasks).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_matrix_names_its_parameter(sq, bad):
    rng = np.random.default_rng(4)
    tasks, layout, vec = _model(rng)
    per_param = {n: [(np.eye(len(order)), order)] for n, (order, D) in layout.items()}
    broken = np.eye(3)
    broken[1, 2] = bad
    per_param["w.1"] = [(broken, layout["w.1"][0])]
    with pytest.raises(ValueError, match=r"'w\.1'"):
        sq.assemble_task_gram(per_param, tasks)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly(sq, tmp_path):
    with pytest.raises(RuntimeError):
        sq.task_gram_from_artifacts({}, {}, device="cuda")
    with pytest.raises(RuntimeError):
        sq.cluster_tasks_from_artifacts({}, {}, 2, device="cuda")
    with pytest.raises(ValueError):      # the method is checked before the device
        sq.cluster_tasks_from_artifacts({}, {}, 2, method="spectral")


def test_remerge_script_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "remerge.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--output-path", "--weighting", "--cluster-k",
                 "--performance-file", "--temperature", "--device"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "add_task.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--weighting" in r.stdout and "--cluster-k" in r.stdout
