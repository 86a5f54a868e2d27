"""
tests/mask_model.py against what the reference itself produced (tests/golden/masks.npz, written by
tests/golden/make_golden.py::gen_masks from the reference's mask_loader.py) and against torch's boolean indexing.
No GPU: the model is the yardstick of tests/test_hip_mask_ops.py, so it is checked where the kernels are not involved.
"""
import math

import numpy as np
import pytest
import torch

import mask_model as mm
from helpers import load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("masks.npz")


def _stack(g, n=None):
    m = g["masks"]
    return m[:n].reshape(m[:n].shape[0], -1)


def test_combine_matches_the_reference(g):
    s = _stack(g)
    assert s.dtype == np.bool_ and s.shape == (5, 2000)
    for strat in mm.STRATEGIES:
        assert np.array_equal(mm.combine(s, strat), g[f"combined_{strat}"].reshape(-1)), strat
    # an even count: a tie passes (the reference's ">= 0.5 * n")
    assert np.array_equal(mm.combine(_stack(g, 4), "majority"), g["majority_even4"].reshape(-1))
    assert (mm.votes(_stack(g, 4)) == 2).any()       # ... and the fixture has ties


def test_threshold_rule_matches_the_reference(g):
    thr = [float(t) for t in g["majority_thresholds"]]
    assert len(thr) == 9
    for n, tag in ((5, "n5"), (3, "n3")):
        s = _stack(g, n)
        for i, t in enumerate(thr):
            want = g[f"majority_thr{i}_{tag}"].reshape(-1)
            assert np.array_equal(mm.majority_threshold(s, t), want), (n, t)
            # the integer form the host layer hands the kernels: the smallest passing count
            need = max(0, min(n + 1, int(math.ceil(float(np.float32(t * n))))))
            assert np.array_equal(mm.combine(s, "majority", votes_needed=need), want), (n, t, need)
        assert np.array_equal(mm.majority_threshold(s, 0.5), mm.combine(s, "majority"))


def test_compact_and_indices_match_the_reference(g):
    union = g["combined_union"].reshape(-1)
    it, if_ = mm.indices(union)
    assert it.size + if_.size == union.size and union[it].all() and not union[if_].any()
    assert np.all(np.diff(it) > 0) and np.all(np.diff(if_) > 0)
    for t, d in enumerate(g["deltas"]):
        sig, noi = mm.compact(d, union)
        assert np.array_equal(sig, g["signal"][t]) and np.array_equal(noi, g["noise"][t])
        assert np.array_equal(sig, d.reshape(-1)[it]) and np.array_equal(noi, d.reshape(-1)[if_])


def test_unpack_inverts_packbits():
    rng = np.random.default_rng(3)
    bits = rng.random(4099) < 0.4
    for pad in range(8):
        stream = np.packbits(np.concatenate([np.zeros(pad, dtype=bool), bits]))
        assert np.array_equal(mm.unpack(stream, pad, bits.size), bits)
        assert np.array_equal(mm.unpack(stream, pad + 5, 9), bits[5:14])
    with pytest.raises(AssertionError):
        mm.unpack(np.packbits(bits), 1, bits.size + 8)


@pytest.mark.parametrize("D,density", [(1, 1.0), (9, 0.5), (2049, 0.03), (5000, 0.5), (5000, 0.97)])
def test_against_torch_boolean_indexing(D, density):
    gen = torch.Generator().manual_seed(D)
    mask = torch.rand(D, generator=gen) < density
    x = torch.randn(D, generator=gen)
    m = mask.numpy()
    it, if_ = mm.indices(m)
    assert np.array_equal(it, torch.nonzero(mask).flatten().numpy())
    assert np.array_equal(if_, torch.nonzero(~mask).flatten().numpy())
    sig, noi = mm.compact(x.numpy(), m)
    assert np.array_equal(sig, x[mask].numpy()) and np.array_equal(noi, x[~mask].numpy())
    stack = torch.stack([torch.rand(D, generator=gen) < 0.5 for _ in range(4)] + [mask])
    v = stack.sum(0)
    assert np.array_equal(mm.combine(stack.numpy(), "union"), (v > 0).numpy())
    assert np.array_equal(mm.combine(stack.numpy(), "intersection"), (v == 5).numpy())
    assert np.array_equal(mm.combine(stack.numpy(), "majority"), (v.float() >= 0.5 * 5).numpy())


def test_unit_starts_model():
    m = np.zeros(10, dtype=bool)
    m[[1, 4, 5, 9]] = True
    assert mm.unit_starts(m, 4, 3, 2, False).tolist() == [1, 5, 10]
    assert mm.unit_starts(m, 2, 2, 2, False).tolist() == [1, 10]            # rows below the count: the plan stops there
    assert mm.unit_starts(m, 9, 3, 2, False).tolist() == [1, 5, 10]         # rows above the count select nothing
    inv = mm.unit_starts(m, 6, 3, 2, True)
    assert [int(v) >> 62 for v in inv] == [1, 1, 1]
    assert [int(v) & (mm.WALK_INV - 1) for v in inv] == [0, 3, 7]
