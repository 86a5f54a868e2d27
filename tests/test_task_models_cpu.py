"""
CPU-only checks of task reconstruction (svdq_task_reconstruct and what is built on it): the new entry points are
declared, exported and bound; without a GPU the callables fail loudly; arguments are validated before any device work;
the script's command line parses.
"""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svdq_task_reconstruct", "svdq_task_reconstruct_work_bytes")


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
    assert len(sq._native.SIGNATURES["svdq_task_reconstruct"][1]) == 12
    # the header cites what the entry does in the reference, as its neighbours do
    doc = header[header.index("every task's OWN reconstruction"):header.index("int64_t svdq_task_reconstruct_work_bytes")]
    assert "merge.py:144-194" in doc and "rtvq.py:85-103" in doc
    # refused without touching a device
    assert lib.svdq_task_reconstruct_work_bytes(None, 8) == 0
    assert lib.svdq_task_reconstruct(None, None, None, None, None, None, 8, None, None, None, None, None) == \
        sq._native.SVDQ_EINVAL
    assert "svdq_task_reconstruct" in sq._native.last_error()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.reconstruct_task_vectors) == [("compressed_all", E), ("bases", E), ("masks", E),
                                                   ("original_shapes", E), ("config", E), ("tasks", None),
                                                   ("device", "cpu"), ("base_state_dict", None)]
    assert sq.reconstruct_task_vectors is sq.merge.reconstruct_task_vectors
    assert params(sq.reconstruct_tasks_from_artifacts) == [("artifact_dir", E), ("base_state_dict", E), ("tasks", None),
                                                           ("output_dir", None), ("device", "cuda")]
    assert params(sq.CompressPlan.reconstruct_tasks)[1:] == [("task_idx", E), ("out_table", E), ("scale", None),
                                                             ("base_table", None), ("rows_dev", None)]


def _dictionaries():
    """Reference-layout dictionaries of one parameter and two tasks (never read without a GPU)."""
    art = {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16),
                      "c_low_quant": {"payloads": [], "num_bits": 4, "num_stages": 2, "original_shape": torch.Size([0]),
                                      "original_dtype": "torch.float32"}}}
    bases = {"w": {"masked": {"U_high": torch.zeros(16, 1, dtype=torch.float16), "U_low": torch.zeros(16, 0, dtype=torch.float16),
                              "singular_values": torch.ones(1), "k": 1, "mean": None, "energy_retained": 1.0, "D": 16,
                              "N": 2}, "noise": None}}
    return {"w": {"A": art, "B": dict(art)}}, bases, {"w": torch.Size([16])}


def test_unknown_task_is_refused_before_any_device_work(sq):
    comp, bases, shapes = _dictionaries()
    with pytest.raises(ValueError, match="'C'"):      # also where no GPU is visible: the names are checked first
        sq.reconstruct_task_vectors(comp, bases, {}, shapes, sq.SVDHybridConfig(), tasks=["A", "C"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_gpu_fails_loudly(sq):
    comp, bases, shapes = _dictionaries()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sq.reconstruct_task_vectors(comp, bases, {}, shapes, sq.SVDHybridConfig())


def test_script_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reconstruct_tasks.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--artifact-dir", "--base-model-path", "--tasks", "--output-dir", "--device"):
        assert flag in r.stdout
