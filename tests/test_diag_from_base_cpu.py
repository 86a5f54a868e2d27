"""
CPU-only checks of the diagnostics from checkpoints (svdq_diagnostics_from_base): the public names, the ctypes
signatures (tests/test_abi_cpu.py then holds them to the header and the exports), the command-line flag, and the
host function that orders the tensors behind the pointer tables.
"""
from ctypes import c_int32, c_void_p

import pytest
import torch


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def test_public_names(sq):
    assert "compute_all_diagnostics_from_checkpoints" in sq.__all__
    assert sq.compute_all_diagnostics_from_checkpoints is sq.diagnostics.compute_all_diagnostics_from_checkpoints
    for name in ("diagnostics_from_base", "diagnostics_masked_from_base"):
        assert callable(getattr(sq.CompressPlan, name))


def test_signatures(sq):
    sig = sq._native.SIGNATURES
    assert sig["svdq_diagnostics_from_base"] == (c_int32, [c_void_p] * 7 + [c_int32] + [c_void_p] * 3)
    assert sig["svdq_diagnostics_masked_from_base"] == (c_int32, [c_void_p] * 9 + [c_int32] + [c_void_p] * 3)
    # one argument more than the calls on materialised deltas: the base table
    assert len(sig["svdq_diagnostics_from_base"][1]) == len(sig["svdq_diagnostics"][1]) + 1
    assert len(sig["svdq_diagnostics_masked_from_base"][1]) == len(sig["svdq_diagnostics_masked"][1]) + 1


def test_command_line_flag(sq):
    common = ["--tasks", "A", "--checkpoint-dir", "x", "--base-model-path", "y"]
    assert sq.cli.parse_args(common).eval_from_checkpoints is False
    args = sq.cli.parse_args(common + ["--eval-from-checkpoints"])
    assert args.eval_from_checkpoints is True and args.eval_reconstruction is True


def test_checkpoint_tables_order_skips_and_refusals(sq):
    from svdq_amd.diagnostics import checkpoint_tables
    base = {"w": torch.zeros(4, 3), "b": torch.zeros(5)}
    ft = {"t1": {"w": torch.ones(4, 3), "b": torch.ones(5)},
          "t0": {"w": torch.full((4, 3), 2.0)},                      # lacks "b"
          "t2": {"w": torch.full((4, 3), 3.0), "b": torch.full((5,), 3.0)}}
    # plan order: entry 0 = "b" with tasks (t2, t0, t1), entry 1 = "w" with tasks (t0, t1, t2)
    tabs, bs = checkpoint_tables(["b", "w"], [["t2", "t0", "t1"], ["t0", "t1", "t2"]], base, ft)
    assert len(tabs) == 6 and len(bs) == 2
    assert bs[0] is base["b"] and bs[1] is base["w"]
    assert tabs[0] is ft["t2"]["b"] and tabs[1] is None and tabs[2] is ft["t1"]["b"]      # the missing pair is skipped
    assert [t is ft[k]["w"] for t, k in zip(tabs[3:], ("t0", "t1", "t2"))] == [True] * 3
    # a task the caller does not pass at all is skipped the same way
    tabs, _ = checkpoint_tables(["w"], [["t9", "t1"]], base, ft)
    assert tabs[0] is None and tabs[1] is ft["t1"]["w"]
    with pytest.raises(ValueError, match="shape"):
        checkpoint_tables(["w"], [["t1"]], base, {"t1": {"w": torch.ones(3, 4)}})
    with pytest.raises(ValueError, match="no base tensor"):
        checkpoint_tables(["q"], [["t1"]], base, ft)


def test_exact_reads_never_narrow(sq):
    from svdq_amd.diagnostics import _exact_for
    f32, f16, bf16 = (torch.zeros(2, dtype=d) for d in (torch.float32, torch.float16, torch.bfloat16))
    assert _exact_for(torch.float32, [f32, f16, bf16, None])          # widening is exact
    assert _exact_for(torch.float16, [f16, f16]) and _exact_for(torch.bfloat16, [bf16])
    assert not _exact_for(torch.float16, [f16, f32])                   # a half plan would have to narrow
    assert not _exact_for(torch.float16, [bf16])
    assert not _exact_for(torch.float32, [torch.zeros(2, dtype=torch.float64)])
