"""CPU tests of the host logic behind svdq_plan_residual_gram / svdq_plan_extend_basis: the agreement of include/svdq.h
with the ctypes binding (signatures and the layout struct), the new flags of scripts/add_task.py, the dictionary surgery
of an extended store (``compress.extended_basis_entry``, ``pad_c_high``) on hand-made dictionaries, and the
``ValueError``s that come before anything runs."""

import ctypes
import inspect
import os
import re
import sys
from ctypes import c_float, c_int32, c_int64, c_void_p

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _basis(D, k, n_low, dtype=torch.float16, N=None):
    return {"U_high": torch.zeros(D, k, dtype=dtype), "U_low": torch.zeros(D, n_low, dtype=dtype),
            "singular_values": torch.ones(k + n_low), "k": k, "mean": torch.zeros(D, 1),
            "energy_retained": 0.9, "D": D, "N": (k + n_low) if N is None else N}


def test_header_binding_and_layout_struct_agree():
    import svdq_amd
    nat = svdq_amd._native
    text = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype_of = {"int32_t": c_int32, "float": c_float}
    for name, ret in (("svdq_plan_residual_gram_work_bytes", "int64_t"), ("svdq_plan_extend_layout", "int"),
                      ("svdq_plan_residual_gram", "int"), ("svdq_plan_extend_basis", "int")):
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert m.group(1) == ret
        params = [a.strip() for a in m.group(2).split(",")]
        res, args = nat.SIGNATURES[name]
        assert res is (c_int64 if ret == "int64_t" else c_int32)
        assert len(args) == len(params), (name, params)
        for a, prm in zip(args, params):
            if "*" in prm:
                assert a is c_void_p or issubclass(a, ctypes._Pointer), (name, prm)
            else:
                assert a is ctype_of[prm.split()[0]], (name, prm)
    # the layout struct, field by field
    m = re.search(r"typedef struct svdq_extend_layout \{(.*?)\} svdq_extend_layout;", code, flags=re.S)
    fields = re.findall(r"int64_t\s+(\w+)\s*;", m.group(1))
    assert fields == [f for f, _ in nat.SvdqExtendLayout._fields_]
    assert all(t is c_int64 for _, t in nat.SvdqExtendLayout._fields_)
    assert int(re.search(r"#define SVDQ_MAX_NEW_TASKS (\d+)", code).group(1)) == nat.MAX_NEW_TASKS == 8
    assert "svdq_abi_version" in code and "#define SVDQ_ABI_VERSION 1" in code
    for meth in ("residual_gram", "extend_basis"):
        assert hasattr(svdq_amd.CompressPlan, meth)
    assert callable(svdq_amd.extend_bases)
    E = inspect.Parameter.empty
    got = [(p.name, p.default) for p in inspect.signature(svdq_amd.extend_bases).parameters.values()]
    assert got == [("task_vectors", E), ("masks", E), ("bases", E), ("config", E), ("device", "cuda"),
                   ("base_state_dict", None), ("min_residual", 2.0 ** -12)]
    tail = list(inspect.signature(svdq_amd.add_tasks_to_artifacts).parameters.values())[-2:]
    assert [(p.name, p.default) for p in tail] == [("extend_basis", False), ("min_residual", 2.0 ** -12)]


def test_add_task_accepts_the_new_flags(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import add_task
    finally:
        sys.path.pop(0)
    ap = add_task.build_parser()
    common = ["--artifact-dir", "a", "--base-model-path", "b", "--checkpoint", "x=y"]
    args = ap.parse_args(common)
    assert args.extend_basis is False and args.min_residual == 2.0 ** -12
    args = ap.parse_args(common + ["--extend-basis", "--min-residual", "0.001"])
    assert args.extend_basis is True and args.min_residual == 0.001
    with pytest.raises(SystemExit):
        ap.parse_args(common + ["--min-residual", "small"])


def test_extended_basis_entry_surgery():
    import svdq_amd  # noqa: F401
    from svdq_amd.basis import compute_energy_spectrum
    from svdq_amd.compress import extended_basis_entry
    D, k, n_low = 12, 2, 3
    b = _basis(D, k, n_low, N=5)
    b["U_high"] = torch.arange(D * k, dtype=torch.float16).reshape(D, k)
    b["singular_values"] = torch.tensor([5.0, 4.0, 3.0, 2.0, 1.0])
    new = torch.cat([b["U_high"], torch.full((D, 2), 0.5, dtype=torch.float16)], dim=1)
    lam = [9.0, 0.25]
    e = extended_basis_entry(b, new, lam, n_added=1)
    assert e["k"] == 4 and e["N"] == 6 and e["D"] == D
    assert e["U_high"] is new and e["U_low"] is b["U_low"] and e["mean"] is b["mean"]
    # [sigma[:k], sqrt(lambda), sigma[k:]]: not descending, the first k' entries are the high columns
    assert torch.equal(e["singular_values"], torch.tensor([5.0, 4.0, 3.0, 0.5, 3.0, 2.0, 1.0]))
    assert e["energy_retained"] == float(compute_energy_spectrum(e["singular_values"])[3])
    want = (25 + 16 + 9 + 0.25) / (25 + 16 + 9 + 0.25 + 9 + 4 + 1)
    assert abs(e["energy_retained"] - want) < 1e-6
    # the stored dictionary is not touched
    assert b["k"] == 2 and b["N"] == 5 and b["singular_values"].numel() == 5 and b["U_high"].shape == (D, 2)
    with pytest.raises(ValueError, match="shape"):
        extended_basis_entry(b, new[:, :3], lam, n_added=1)
    # k = 0: the new columns become the whole high part
    b0 = _basis(D, 0, 3, N=3)
    e0 = extended_basis_entry(b0, torch.zeros(D, 1, dtype=torch.float16), [4.0], n_added=2)
    assert e0["k"] == 1 and e0["N"] == 5 and torch.equal(e0["singular_values"], torch.tensor([2.0, 1.0, 1.0, 1.0]))


def test_old_tasks_c_high_is_zero_padded():
    import svdq_amd  # noqa: F401
    from svdq_amd.compress import pad_c_high
    q = {"num_bits": 4, "payloads": []}
    art = {"c_high_fp16": torch.tensor([1.5, -2.0], dtype=torch.float16), "c_low_quant": q}
    out = pad_c_high(art, 3)
    assert out["c_high_fp16"].dtype is torch.float16
    assert torch.equal(out["c_high_fp16"], torch.tensor([1.5, -2.0, 0, 0, 0], dtype=torch.float16))
    assert out["c_low_quant"] is q                      # c_low is untouched
    assert art["c_high_fp16"].numel() == 2              # and so is the stored artifact
    assert pad_c_high(art, 0) is art and pad_c_high(None, 2) is None
    empty = pad_c_high({"c_high_fp16": torch.zeros(0, dtype=torch.float16), "c_low_quant": q}, 2)
    assert torch.equal(empty["c_high_fp16"], torch.zeros(2, dtype=torch.float16))


def test_refusals_before_anything_runs():
    import svdq_amd
    from svdq_amd.compress import check_extension_room
    ok = {"p": {"masked": _basis(100, 4, 4, N=8), "noise": None}}
    check_extension_room(ok, 8, 24)
    with pytest.raises(ValueError, match="k \\+ new tasks"):
        check_extension_room({"p": {"masked": _basis(100, 30, 0, N=30)}}, 3)
    with pytest.raises(ValueError, match="r \\+ new tasks"):
        check_extension_room({"p": {"masked": _basis(100, 2, 28, N=30)}}, 3)
    with pytest.raises(ValueError, match="at most 32 tasks in total"):
        check_extension_room({"p": {"masked": _basis(100, 2, 2, N=31)}}, 2)
    with pytest.raises(ValueError, match="at most 32 tasks in total"):
        check_extension_room(ok, 2, 31)
    # a noise region is checked like the masked one
    with pytest.raises(ValueError, match="noise"):
        check_extension_room({"p": {"masked": _basis(100, 1, 1), "noise": _basis(50, 30, 1, N=8)}}, 2)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="1 to 8 new tasks"):
            check_extension_room(ok, bad)
    # the public entry point refuses an over-long task list before it looks at a tensor or a GPU
    cfg = svdq_amd.SVDHybridConfig()
    tasks = {f"t{i}": {"p": None} for i in range(9)}
    with pytest.raises(ValueError, match="1 to 8 new tasks"):
        svdq_amd.extend_bases(tasks, None, ok, cfg)
    with pytest.raises(ValueError, match="1 to 8 new tasks"):
        svdq_amd.extend_bases({}, None, ok, cfg)
    with pytest.raises(ValueError, match="k \\+ new tasks"):
        svdq_amd.extend_bases({"t": {"p": None}}, None, {"p": {"masked": _basis(100, 32, 0, N=32)}}, cfg)
