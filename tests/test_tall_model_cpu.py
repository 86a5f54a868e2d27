"""
tests/tall_model.py against answers worked out by hand: the numpy model is the truth of the GPU tests of the TALL masks
and the consensus merge, so its own rules -- the strict comparison, the zero row, the task that lacks a parameter, the
consensus threshold, the packing -- are pinned here without a GPU.
"""
import numpy as np
import pytest
import torch

import tall_model as tm

# 4 rows x 3 tasks, lambda = 0.5.  Task 2 lacks the parameter of rows 2 and 3 (its values there must not be read).
#   row 0: v = (4, 1, 1), S = 6: task 0: 4 > 0.5 * 2 set; task 1: 1 > 0.5 * 5 no; task 2: no           -> c = 1
#   row 1: v = (2, 4, 0), S = 6: task 0: 2 > 0.5 * 4 is an exact TIE, strict: no; task 1: 4 > 1 set;
#          task 2: 0 > 3 no                                                                              -> c = 1
#   row 2: v = (0, 0, -), S = 0: 0 > 0 is false for both                                                -> c = 0
#   row 3: v = (3, -2, -), S = 1: task 0: 3 > 0.5 * |-2| set; task 1: 2 > 0.5 * 3 set                   -> c = 2
V = np.array([[4, 2, 0, 3], [1, 4, 0, -2], [1, 0, 9, 7]], dtype=np.float32)
HAS = np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 0, 0]], dtype=bool)
MASKS = np.array([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 0, 0]], dtype=bool)
S = np.array([6, 6, 0, 1], dtype=np.float32)


def test_the_hand_computed_case():
    assert np.array_equal(tm.task_sum(V, HAS), S)
    assert np.array_equal(tm.tall_masks(V, HAS, 0.5), MASKS)
    for k, want in ((0, S), (1, [6, 6, 0, 1]), (2, [0, 0, 0, 1]), (3, [0, 0, 0, 0])):
        out, m, stats = tm.consensus_merge(V, HAS, 0.5, k)
        assert out.dtype == np.float32 and np.array_equal(out, np.asarray(want, dtype=np.float32)), k
        assert np.array_equal(m, MASKS)
        assert stats["active"].tolist() == [2, 2, 0] and stats["agreement"].tolist() == [1, 2, 1, 0]
        assert stats["rows"] == 4
    out, _, _ = tm.consensus_merge(V, HAS, 0.5, 1, scaling=0.5, base=np.array([10, 20, 30, 40], dtype=np.float32))
    assert out.tolist() == [13.0, 23.0, 30.0, 40.5]
    # a hair under the tie sets the bit: the comparison is strict, not tolerant
    assert tm.tall_masks(V, HAS, np.nextafter(np.float32(0.5), np.float32(0)))[0, 1]
    # lambda 0 marks every non-zero value a task has; per-task lambdas act per task
    assert np.array_equal(tm.tall_masks(V, HAS, 0.0), (V != 0) & HAS)
    assert np.array_equal(tm.tall_masks(V, HAS, [0.5, 100.0, 0.0]), [[1, 0, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0]])
    # one task: the mask is v != 0
    one = np.array([[0.0, -0.0, 1e-30, -3.0]], dtype=np.float32)
    assert tm.tall_masks(one, None, 0.4).tolist() == [[False, False, True, True]]


def test_k_zero_is_the_sequential_sum_and_k_past_the_task_count_is_refused():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((5, 1000)).astype(np.float32) * np.float32(1e3)
    s = np.zeros(1000, dtype=np.float32)
    for g in range(5):
        s = s + v[g]      # float32 + float32, rounded per step
    out, _, _ = tm.consensus_merge(v, None, 0.4, 0)
    assert np.array_equal(out.view(np.uint32), s.view(np.uint32))
    assert not np.array_equal(out, v.sum(axis=0, dtype=np.float64).astype(np.float32))      # not a wider sum
    for bad in (6, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            tm.consensus_merge(v, None, 0.4, bad)
    for bad in (-0.1, float("nan"), float("inf"), [0.4] * 4):
        with pytest.raises(ValueError, match="tall_lambda"):
            tm.tall_masks(v, None, bad)


def test_streams_are_packbits_of_the_concatenated_bools():
    rng = np.random.default_rng(5)
    a, b = rng.random((3, 13)) < 0.5, rng.random((3, 20)) < 0.5
    streams = tm.pack_streams({"a": a, "b": b}, {"a": 5, "b": 5 + 13}, 5 + 13 + 20)
    lead = np.zeros((3, 5), dtype=bool)
    assert streams.dtype == np.uint8 and streams.shape == (3, 5)
    for g in range(3):
        assert np.array_equal(streams[g], np.packbits(np.concatenate([lead[g], a[g], b[g]])))
    # stream bit i is bit 7 - (i & 7) of byte i >> 3
    only = np.zeros((1, 38), dtype=bool)
    only[0, 11] = True
    assert tm.pack_streams({"x": only}, {"x": 0}, 38)[0].tolist() == [0, 1 << (7 - 3), 0, 0, 0]
    with pytest.raises(ValueError, match="outside the stream"):
        tm.pack_streams({"a": a}, {"a": 30}, 38)


def test_a_stream_unpacks_through_vector_to_state_dict():
    import svdq_amd
    ref = {"a.skip": torch.zeros(5), "b": torch.zeros(13), "c": torch.zeros(4, 5)}
    rng = np.random.default_rng(7)
    b, c = rng.random((2, 13)) < 0.5, rng.random((2, 20)) < 0.5
    streams = tm.pack_streams({"b": b, "c": c}, {"b": 5, "c": 18}, 38)
    for g in range(2):
        bits = torch.from_numpy(np.unpackbits(streams[g])[:38].copy())
        got = svdq_amd.vector_to_state_dict(bits, ref)
        assert not got["a.skip"].any()
        assert np.array_equal(got["b"].numpy().astype(bool), b[g])
        assert got["c"].shape == (4, 5) and np.array_equal(got["c"].numpy().astype(bool).reshape(-1), c[g])
