"""
CPU-only checks of masked task reconstruction inside the streaming pass (svdq_task_reconstruct_masked and what is built
on it): the entry point is declared, exported and bound and refuses bad arguments without a device; the eligibility
predicate the merge and the task reconstruction share, one case per decline reason; the mask-count check of the
adoption helper; the script's command line.
"""
import importlib.util
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "svdq_task_reconstruct_masked"


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd


def test_entry_point_is_declared_exported_and_bound(sq):
    header = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sq._native.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T svdq_" in ln}
    lib = sq._native.lib()
    assert re.search(rf"\b{NAME}\s*\(", code)
    assert NAME in exported and NAME in sq._native.SIGNATURES and hasattr(lib, NAME)
    assert len(sq._native.SIGNATURES[NAME][1]) == 15
    assert lib.svdq_abi_version() == 1
    # the one statement of the contract sits below svdq_merge_masked and cites what the entry does in the reference
    at = header.index("int svdq_merge_masked(")
    doc = header[at:header.index(f"int {NAME}(")]
    for cite in ("mask_loader.py:712-763", "rtvq.py:85-103", "merge.py:144-194", "merge.py:429-552"):
        assert cite in doc, cite
    # refused without touching a device
    assert getattr(lib, NAME)(*([None] * 6), 8, *([None] * 8)) == sq._native.SVDQ_EINVAL
    assert NAME in sq._native.last_error()


def test_python_surface(sq):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(sq.CompressPlan.reconstruct_tasks_masked)[1:] == [
        ("task_idx", E), ("mask_table", E), ("unit_start", E), ("rows_dev", E), ("out_table", E), ("scale", None),
        ("fill", None), ("base_table", None)]
    # the keyword lives on functions of its own; the two they extend keep their signatures and are the same call without it
    assert params(sq.reconstruct_task_vectors_masked) == params(sq.reconstruct_task_vectors) + [("fused_masks", True)]
    assert params(sq.reconstruct_tasks_from_artifacts_masked) == [
        ("artifact_dir", E), ("base_state_dict", E), ("masks", E), ("tasks", None), ("output_dir", None),
        ("device", "cuda"), ("fused_masks", True)]
    assert "fused_masks" not in dict(params(sq.reconstruct_task_vectors))
    assert "masks" not in dict(params(sq.reconstruct_tasks_from_artifacts))
    assert sq.reconstruct_task_vectors_masked is sq.merge.reconstruct_task_vectors_masked
    with pytest.raises(ValueError, match="'C'"):      # names are checked before any device work, as in the function it extends
        sq.reconstruct_task_vectors_masked({"w": {"A": {}, "B": {}}}, {}, {}, {}, sq.SVDHybridConfig(), tasks=["A", "C"])
    assert params(sq.adopt_artifacts)[-1] == ("masks", None)
    assert not hasattr(torch.ops, "svdq") or not hasattr(torch.ops.svdq, "task_reconstruct_masked")


# ------------------------------------------------------------------------------------------ the shared predicate
def _batch(mode="walk", ident=None, unit_start=object()):
    return SimpleNamespace(mode=mode, mask_ident=({} if ident is None else {"w": ident}), unit_start=unit_start)


def test_source_walk_predicate_one_case_per_decline_reason(sq):
    from svdq_amd import merge as mg
    mask = torch.ones(16, dtype=torch.bool)
    ident = mg._mask_identity(mask)
    ok = _batch(ident=ident)
    assert mg._source_walk_decline(ok, None, "w", mask) is None
    assert mg._source_walk_decline(ok, _batch("gather", ident), "w", mask) is None
    reasons = [
        mg._source_walk_decline(_batch("plain", ident), None, "w", mask),            # a plain (or adopted) batch
        mg._source_walk_decline(_batch(), None, "w", mask),                          # no mask recorded for the name
        mg._source_walk_decline(ok, None, "w", mask.clone()),                        # another mask object
        mg._source_walk_decline(ok, None, "w", None),                                # no mask at all
        mg._source_walk_decline(_batch(ident=ident, unit_start=None), None, "w", mask),
        mg._source_walk_decline(ok, _batch("gather", ident, unit_start=None), "w", mask),
        mg._source_walk_decline(ok, _batch("gather", mg._mask_identity(mask.clone())), "w", mask),
        mg._source_walk_decline(ok, _batch("gather"), "w", mask),                    # the noise batch has no record
    ]
    assert all(isinstance(r, str) and r for r in reasons), reasons
    assert len({reasons[i] for i in (0, 1, 2, 4, 5, 6)}) == 6      # each reason is told apart
    # a batch without the attributes at all (an older object) declines like a plain one
    assert mg._source_walk_decline(SimpleNamespace(), None, "w", mask) == reasons[0]
    # _merge_batched uses this very predicate
    assert "_source_walk_decline(" in inspect.getsource(mg._merge_batched)
    assert "_source_walk_decline(" in inspect.getsource(mg._task_walk_plans)


# ------------------------------------------------------------------------------------------ the adoption helper
def test_mask_counts_must_equal_the_stored_rows(sq):
    from svdq_amd.driver import _planned_rows, _walk_usable
    entries = [("a", "masked"), ("a", "noise"), ("b", "masked"), ("c", "masked"), ("d", "masked"), ("e", "noise")]
    q_of = {"a": 0, "b": 1, "d": 2, "e": 3}      # "c" comes without a mask
    numels = [100, 50, 80, 40]
    ct, cf = [60, 30, 41, 25], [40, 20, 39, 15]
    plan_rows = [100, 100, 50, 70, 80, 40]
    #            a/masked fits, a/noise fits, b one short, c no mask, d: one more set element, e fits
    stored = [60, 40, 29, 70, 40, 15]
    assert _walk_usable(entries, q_of, plan_rows, stored, numels, ct, cf) == [0, 1, 5]
    # the plan must hold the mask's element count as its source rows (adopt_artifacts(..., masks=...))
    assert _walk_usable(entries, q_of, [60, 40, 29, 70, 40, 15], stored, numels, ct, cf) == []
    # an entry without rows is never walked
    assert _walk_usable(entries, q_of, plan_rows, [0, 40, 29, 70, 40, 15], numels, ct, cf) == [1, 5]
    # polarity: the noise entry counts the cleared elements
    assert _walk_usable([("a", "noise")], q_of, [100], [60], numels, ct, cf) == []
    basis = {"U_high": torch.zeros(60, 1)}
    e = {"name": "a", "basis": basis}
    assert _planned_rows(e, None) == 60 and _planned_rows(e, {}) == 60
    assert _planned_rows(e, {"a": torch.ones(100, dtype=torch.bool)}) == 100
    assert _planned_rows(e, {"a": torch.ones(10, 10, dtype=torch.bool)}) == 100
    assert _planned_rows(e, {"a": torch.ones(59, dtype=torch.bool)}) == 60      # a mask smaller than the stored rows


# ------------------------------------------------------------------------------------------ the script
def _script():
    spec = importlib.util.spec_from_file_location("reconstruct_tasks_script",
                                                  os.path.join(ROOT, "scripts", "reconstruct_tasks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_arguments():
    mod = _script()
    need = ["--artifact-dir", "a", "--base-model-path", "b.pt", "--output-dir", "o"]
    args = mod.build_parser().parse_args(need)
    assert args.mask_dir is None and args.mask_strategy is None and args.device == "cuda"
    args = mod.build_parser().parse_args(need + ["--mask-dir", "m", "--mask-strategy", "majority", "--tasks", "x", "y"])
    assert (args.mask_dir, args.mask_strategy, args.tasks) == ("m", "majority", ["x", "y"])
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(need + ["--mask-dir", "m", "--mask-strategy", "xor"])
    with pytest.raises(SystemExit):      # a strategy without masks means nothing: refused before anything is loaded
        mod.main(need + ["--mask-strategy", "union"])
    text = mod.build_parser().format_help()
    assert "--mask-dir" in text and "--mask-strategy" in text
