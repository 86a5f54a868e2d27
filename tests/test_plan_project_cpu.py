"""CPU tests of the host logic behind svdq_plan_project: the grouping and slot count of driver.adopt_bases
(``_bases_plan_specs``, shapes and dtypes only), the argument checking of scripts/add_task.py, and the agreement of
include/svdq.h with the ctypes binding for the new symbols."""

import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _basis(D, k, n_low, dtype=torch.float16, mean=True):
    return {"U_high": torch.zeros(D, k, dtype=dtype), "U_low": torch.zeros(D, n_low, dtype=dtype),
            "singular_values": torch.ones(k + n_low), "k": k, "mean": torch.zeros(D, 1) if mean else None,
            "energy_retained": 0.9, "D": D, "N": k + n_low}


def test_adopt_bases_groups_and_slot_count():
    import svdq_amd  # noqa: F401
    from svdq_amd.driver import _bases_plan_specs
    bases = {
        "a": {"masked": _basis(100, 2, 6), "noise": _basis(50, 1, 4)},
        "b": {"masked": _basis(300, 3, 2)},
        "c": {"masked": _basis(64, 1, 1, dtype=torch.float32)},
        "d": {"masked": _basis(64, 1, 1, mean=False)},
        "e": {"masked": _basis(5, 2, 3)},
    }
    specs, declined = _bases_plan_specs(bases, 1)
    assert declined == {}
    by_key = {(s["udt"], s["no_mean"]): s for s in specs}
    assert set(by_key) == {(torch.float16, False), (torch.float32, False), (torch.float16, True)}
    main = by_key[(torch.float16, False)]
    # both regions of a parameter are entries of their own, in the dictionaries' order
    assert [(e["name"], e["region"]) for e in main["entries"]] == [("a", "masked"), ("a", "noise"), ("b", "masked"),
                                                                   ("e", "masked")]
    assert main["N"] == 8                                   # one new task, but the largest stored r is 8: r <= N holds
    assert by_key[(torch.float32, False)]["N"] == 2 and by_key[(torch.float16, True)]["N"] == 2
    specs12, _ = _bases_plan_specs(bases, 12)
    assert {s["N"] for s in specs12} == {12}                # room for every new task
    for bad in (0, 33):
        with pytest.raises(ValueError, match="n_slots"):
            _bases_plan_specs(bases, bad)


def test_adopt_bases_declines_what_a_plan_cannot_hold():
    import svdq_amd  # noqa: F401
    from svdq_amd.driver import _bases_plan_specs
    wide = _basis(100, 20, 13)                               # r = 33 > 32 slots
    short = _basis(4, 3, 2)                                  # r = 5 > D = 4
    odd = _basis(10, 1, 1)
    odd["U_low"] = odd["U_low"].double()
    nok = _basis(10, 2, 1)
    nok["k"] = 1
    bases = {"wide": {"masked": wide}, "short": {"masked": short}, "odd": {"masked": odd}, "k": {"masked": nok},
             "none": {"masked": None}, "ok": {"masked": _basis(10, 1, 1)},
             "half": {"masked": _basis(10, 1, 1), "noise": short}}
    specs, declined = _bases_plan_specs(bases, 3)
    assert sorted(declined) == ["half", "k", "none", "odd", "short", "wide"]      # a parameter goes with ALL its regions
    assert [(e["name"], e["region"]) for s in specs for e in s["entries"]] == [("ok", "masked")]
    assert specs[0]["N"] == 3


def test_adopt_artifacts_groups_are_what_they_were():
    """The refactoring that lets adopt_bases share the grouping leaves adopt_artifacts' keys alone."""
    import svdq_amd  # noqa: F401
    from svdq_amd.driver import _adoption_groups
    art = {"c_high_fp16": torch.zeros(2, dtype=torch.float16),
           "c_low_quant": {"num_bits": 4, "num_stages": 2, "original_shape": torch.Size([1]), "original_dtype": "torch.float32",
                           "payloads": [{"stage": s, "quantized": torch.zeros(1, dtype=torch.uint8),
                                         "scale": torch.tensor(1.0), "zero_point": torch.tensor(0.0),
                                         "residual_norm": 0.0} for s in range(2)]}}
    bases = {"p": {"masked": _basis(10, 2, 1)}}
    comp = {"p": {t: {"masked": art, "unmasked": None} for t in ("x", "y", "z")}}
    groups, declined = _adoption_groups(bases, comp)
    assert declined == {} and list(groups) == [(3, 2, torch.float16, False)]
    e = groups[(3, 2, torch.float16, False)][0]
    assert (e["name"], e["region"], e["tasks"], e["bits"]) == ("p", "masked", ["x", "y", "z"], 4)


def _add_task():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import add_task
    finally:
        sys.path.pop(0)
    return add_task


def test_add_task_arguments(tmp_path, capsys):
    add_task = _add_task()
    ap = add_task.build_parser()
    base, ck = tmp_path / "base.pt", tmp_path / "ft.pt"
    base.write_bytes(b"")
    ck.write_bytes(b"")
    args = ap.parse_args(["--artifact-dir", "a", "--base-model-path", str(base), "--checkpoint", f"dtd={ck}",
                          "--checkpoint", f"cars={ck}", "--mask-dir", "m", "--output-dir", "o", "--weights-json", "w.json"])
    assert (args.artifact_dir, args.mask_dir, args.output_dir, args.weights_json) == ("a", "m", "o", "w.json")
    assert add_task.parse_checkpoints(ap, args.checkpoint) == {"dtd": str(ck), "cars": str(ck)}
    assert ap.parse_args(["--artifact-dir", "a", "--base-model-path", "b", "--checkpoint", "x=y"]).output_dir is None
    common = ["--artifact-dir", "a", "--base-model-path", str(base)]
    for bad in (common,                                                        # no checkpoint at all
                common + ["--checkpoint", "nopath"], common + ["--checkpoint", "=p"], common + ["--checkpoint", "n="],
                common + ["--checkpoint", f"n={ck}", "--checkpoint", f"n={ck}"],      # a name twice
                common + ["--checkpoint", f"n={tmp_path / 'missing.pt'}"],            # files are looked at before any work
                ["--artifact-dir", "a", "--base-model-path", str(tmp_path / "nobase.pt"), "--checkpoint", f"n={ck}"],
                ["--base-model-path", str(base), "--checkpoint", f"n={ck}"]):         # no artifact directory
        with pytest.raises(SystemExit) as exc:
            add_task.main(bad)
        assert exc.value.code == 2, bad
    capsys.readouterr()
    wj = tmp_path / "w.json"
    wj.write_text("[1, 2]")
    with pytest.raises(SystemExit) as exc:
        add_task.main(common + ["--checkpoint", f"n={ck}", "--weights-json", str(wj)])
    assert exc.value.code == 2


def test_header_and_binding_agree_on_the_new_symbols():
    from ctypes import c_int32, c_int64, c_void_p
    import svdq_amd
    text = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sig = svdq_amd._native.SIGNATURES
    for name, ret in (("svdq_plan_project_work_bytes", "int64_t"), ("svdq_plan_project", "int")):
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert m.group(1) == ret
        params = [a.strip() for a in m.group(2).split(",")]
        res, args = sig[name]
        assert res is (c_int64 if ret == "int64_t" else c_int32)
        assert len(args) == len(params), (name, params)
        assert all(a is c_void_p for a in args) and all("*" in a for a in params)
    # the contract cites the reference lines it replaces
    assert "compress.py:6-56" in text and "compress.py:173-207" in text
    assert hasattr(svdq_amd.CompressPlan, "project_tasks")
    for fn in ("project_all_parameters", "adopt_bases", "add_tasks_to_artifacts"):
        assert callable(getattr(svdq_amd, fn)), fn
