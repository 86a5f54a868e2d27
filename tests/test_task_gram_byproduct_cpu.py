"""
Host side of the task-Gram by-product, without a GPU: the scatter of a plan's Gram into the run's N x N matrix, the
record look-up, argument validation, unchanged defaults of the public functions, and the shape of the native sources
(the new pass-1 variant exists for plain deltas and minus-base only; the ABI names the two new entry points).
"""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "svd-quantization-task-merging_amd")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _gram(X):
    return X @ X.T


def test_scatter_two_tasks(sq):
    tasks = ["a", "b"]
    X = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 4.0]])
    G = np.zeros((2, 2))
    sq.clustering.scatter_task_gram(G, _gram(X), ["a", "b"], tasks)
    np.testing.assert_array_equal(G, _gram(X))
    # the plan saw the tasks in the other order
    G = np.zeros((2, 2))
    sq.clustering.scatter_task_gram(G, _gram(X[::-1]), ["b", "a"], tasks)
    np.testing.assert_array_equal(G, _gram(X))


def test_scatter_three_tasks_one_missing(sq):
    tasks = ["a", "b", "c"]                      # sorted-name order of the run
    rng = np.random.default_rng(0)
    P1 = rng.standard_normal((3, 5))             # parameter 1: all tasks, plan order c, a, b
    P2 = rng.standard_normal((2, 7))             # parameter 2: task b lacks it; plan order c, a
    G = np.zeros((3, 3))
    sq.clustering.scatter_task_gram(G, _gram(P1), ["c", "a", "b"], tasks)
    sq.clustering.scatter_task_gram(G, _gram(P2), ["c", "a"], tasks)
    full = np.zeros((3, 12))                     # flatten_task_vectors: zeros where a task lacks a parameter
    full[[2, 0, 1], :5] = P1
    full[[2, 0], 5:] = P2
    np.testing.assert_allclose(G, _gram(full), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(G[1, :], _gram(full)[1, :])


class _Art(dict):
    def __init__(self, batch):
        super().__init__()
        self._batch = (batch, 0)


class _Batch:
    def __init__(self, rec):
        self.task_gram = rec


def test_recorded_task_gram(sq):
    rec1 = {"gram": np.array([[2.0, 1.0], [1.0, 3.0]]), "tasks": ["t1", "t0"], "names": ["w", "v"]}
    rec2 = {"gram": np.array([[5.0]]), "tasks": ["t0"], "names": ["u"]}
    b1, b2 = _Batch(rec1), _Batch(rec2)
    bases = {"w": {"masked": _Art(b1), "noise": None}, "v": {"masked": _Art(b1), "noise": None},   # one plan, two names
             "u": {"masked": _Art(b2), "noise": None}, "m": {"masked": _Art(_Batch(None)), "noise": None},
             "plain": {"masked": {"k": 1}, "noise": None}}
    G, covered = sq.clustering.recorded_task_gram(bases, ["t0", "t1"])
    np.testing.assert_array_equal(G, np.array([[3.0 + 5.0, 1.0], [1.0, 2.0]]))
    assert covered == {"w", "v", "u"}
    # the record does not fit the task set, or there is none: today's route
    assert sq.clustering.recorded_task_gram(bases, ["t0", "t2"]) is None
    assert sq.clustering.recorded_task_gram({"plain": {"masked": {"k": 1}, "noise": None}}, ["t0"]) is None
    assert sq.clustering.recorded_task_gram({}, ["t0"]) is None


def test_keyword_defaults(sq):
    for fn in (sq.clustering.task_gram, sq.clustering.cluster_tasks, sq.clustering.compute_cluster_statistics):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "bases" and p["bases"].default is None, fn.__name__
    for fn in (sq.driver.build_bases, sq.driver.run_basis_and_compress,
               sq.driver.run_basis_and_compress_from_checkpoints):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "task_gram" and p["task_gram"].default is None, fn.__name__
    p = inspect.signature(sq.pipeline.CompressPlan.__init__).parameters
    assert p["task_gram"].default is False and p["task_gram"].kind is inspect.Parameter.KEYWORD_ONLY
    # positional calls of the reference's signatures still bind as before
    inspect.signature(sq.cluster_tasks).bind({}, 2, "kmeans")
    inspect.signature(sq.compute_cluster_statistics).bind({}, {})


def test_plan_argument_validation(sq):
    # refused before anything touches the library or the device
    with pytest.raises(ValueError, match="task_gram"):
        sq.pipeline.CompressPlan([16], 2, gram_only=True, task_gram=True)


def test_abi_names_and_version(sq):
    nat = sq._native
    assert "svdq_plan_set_task_gram" in nat.SIGNATURES and "svdq_plan_task_gram" in nat.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "svdq.h")).read()
    assert re.search(r"#define SVDQ_ABI_VERSION 1\b", hdr)
    assert "clustering.py:55-120" in hdr and ":198-245" in hdr and ":263-316" in hdr


def test_side_variant_instantiated_for_plain_and_minus_base_only():
    src = open(os.path.join(PKG, "csrc", "svdq_gram.hip")).read()
    assert "static_assert(!SIDE || (MODE & ~2) == 0" in src
    body = src[src.index("static int launch_gram_side"):src.index("// Variants: the walk")]
    assert "svdq_dispatch_int<0, 2>(in.mode()" in body and "k_gram_side<NTP, MODE, F64, FULL, TIN>" in body
    # the launcher of the existing kernels still instantiates k_gram alone
    rest = src[src.index("int svdq_launch_gram("):]
    assert rest.count("k_gram_side") == 0 and "k_gram<NTP, MODE, F64, FULL, TIN>" in rest


def test_library_cross_compiles_with_the_new_exports(sq):
    import subprocess
    path = sq._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ("svdq_plan_set_task_gram", "svdq_plan_task_gram"):
        assert re.search(rf"\bT {name}\b", out), name
