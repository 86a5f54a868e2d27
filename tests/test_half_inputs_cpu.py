"""
Host-side rules of the fp16 / bf16 input route (no GPU): which task tensors a plan reads as they are and which are
converted to fp32 first, how a half tensor is prepared, and that the new ABI entry point is declared, exported and
bound together.
"""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    if not os.path.exists(svdq_amd._native.LIB_PATH):
        svdq_amd._native.build()
    return svdq_amd


def _t(dtype, n=16):
    return torch.zeros(n, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_one_half_dtype_goes_native(sq, dtype):
    nd = sq.pipeline.native_input_dtype
    assert nd([_t(dtype) for _ in range(5)]) is dtype
    assert nd(iter([_t(dtype), _t(dtype)])) is dtype          # any iterable
    assert nd([_t(dtype), None, _t(dtype)]) is dtype          # an absent base tensor does not count


@pytest.mark.parametrize("tensors", [
    [torch.float32, torch.float32],
    [torch.float16, torch.bfloat16],
    [torch.bfloat16, torch.float32],
    [torch.float16, torch.float16, torch.float32],            # the base tensor of a from-base group in fp32
    [torch.float64, torch.float64],
    [],
])
def test_mixed_or_other_dtypes_upcast(sq, tensors):
    assert sq.pipeline.native_input_dtype([_t(d) for d in tensors]) is torch.float32


def test_prepare_input_keeps_half_tensors(sq):
    pi = sq.pipeline.prepare_input
    x = torch.randn(6, 8).to(torch.bfloat16)
    v = pi(x, CPU, torch.bfloat16)
    assert v.dtype is torch.bfloat16 and v.dim() == 1 and v.data_ptr() == x.data_ptr()     # a view, no copy
    flat = torch.randn(64).to(torch.float16)
    assert pi(flat, CPU, torch.float16) is not None and pi(flat, CPU, torch.float16).data_ptr() == flat.data_ptr()
    # storage offset 1 (2 bytes): not 8-byte aligned -> cloned, same values
    mis = flat[1:]
    assert mis.data_ptr() % 8 != 0
    w = pi(mis, CPU, torch.float16)
    assert w.data_ptr() % 8 == 0 and torch.equal(w, mis)
    # non-contiguous: made contiguous, values kept
    nc = torch.randn(8, 6).to(torch.float16).t()
    assert torch.equal(pi(nc, CPU, torch.float16), nc.contiguous().view(-1))
    with pytest.raises(ValueError):
        pi(flat, CPU, torch.bfloat16)


def test_prepare_input_float32_is_prepare_vector(sq):
    x = torch.randn(5, 7).to(torch.bfloat16)
    a = sq.pipeline.prepare_input(x, CPU, torch.float32)
    b = sq.pipeline.prepare_vector(x, CPU)
    assert a.dtype is torch.float32 and torch.equal(a, b) and torch.equal(a, x.float().view(-1))


def test_compress_plan_rejects_unknown_input_dtype(sq):
    with pytest.raises(ValueError):
        sq.pipeline.CompressPlan([256], 2, input_dtype=torch.float64, device="cpu")


def test_input_type_codes_match_header(sq):
    text = open(os.path.join(ROOT, "include", "svdq.h")).read()
    m = re.search(r"SVDQ_INPUT_F32\s*=\s*(\d+),\s*SVDQ_INPUT_F16\s*=\s*(\d+),\s*SVDQ_INPUT_BF16\s*=\s*(\d+)", text)
    assert m, "input type enum missing from include/svdq.h"
    nat = sq._native
    assert tuple(int(x) for x in m.groups()) == (nat.SVDQ_INPUT_F32, nat.SVDQ_INPUT_F16, nat.SVDQ_INPUT_BF16)
    assert sq.pipeline.INPUT_TYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_set_input_type_declared_exported_and_bound(sq):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svdq.h")).read(), flags=re.S)
    assert re.search(r"int\s+svdq_plan_set_input_type\s*\(\s*svdq_plan\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sq._native.LIB_PATH], text=True)
    assert any(ln.split()[-1] == "svdq_plan_set_input_type" for ln in out.splitlines() if " T " in ln)
    from ctypes import c_int32, c_void_p
    assert sq._native.SIGNATURES["svdq_plan_set_input_type"] == (c_int32, [c_void_p, c_int32])
    assert sq._native.lib().svdq_abi_version() == 1
