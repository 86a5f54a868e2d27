"""
The numpy model of the register form of pass 1 (tests/gram_registers_model.py) against an fp64 numpy Gram of the same
centred fp32 rows, within the forward-error bound of an fp64 sum of D exact terms, (D - 1) 2^-53 sum |x_i x_j| per entry
(derived in gram_registers_model.gram_reference, not fitted), and the properties the device test leans on: the lane ->
row map, the unit and chunk decomposition, the zeros of the second slot, and that a dropped row is far outside the bound.
"""
import numpy as np
import pytest

import gram_registers_model as gm
from oracle import svd_hybrid_oracle as orc

TASKS = [1, 3, 4, 5, 7, 8]
ROWS = [1, 3, 255, 256, 257, 4095, 4097, 8193]
UNIT_ROWS = 4096


def _rows(D, N, seed, center):
    deltas = gm.spiked_deltas([d.numpy() for d in orc.synthetic_deltas(D, N, seed, rank=min(3, N))])
    return gm.centre(deltas, center)


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("N", TASKS)
def test_model_within_fp64_sum_bound(N, center):
    worst = 0.0
    for i, D in enumerate(ROWS):
        xc = _rows(D, N, 700 + i, center)
        got = gm.gram_total(gm.gram_chunks(xc, UNIT_ROWS))
        want, bound = gm.gram_reference(xc)
        err = np.abs(got - want)
        assert np.all(err <= bound), (N, D, center, float((err - bound).max()))
        assert np.array_equal(got, got.T)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"gram registers model N={N} center={center}: worst error / bound {worst:.3g}")


def test_lane_owns_four_consecutive_rows():
    """One nonzero row r: only lane (r % 256) / 4 has a sum, and the unit's partial is that row's outer product."""
    N = 5
    for r in (0, 3, 4, 255, 256, 1023):
        xc = np.zeros((1024, N), dtype=np.float32)
        xc[r] = np.arange(1, N + 1, dtype=np.float32) * np.float32(0.37)
        want = np.outer(xc[r].astype(np.float64), xc[r].astype(np.float64))
        assert np.array_equal(gm.unit_partial(xc), want), r


def test_order_inside_a_lane_and_across_lanes():
    """Three rows whose squares are 4 and twice s = 25 * 2^-56 (0.39 ulp of 4).  Added one after the other to 4, both s
    are lost; added to each other first, 2 s = 0.78 ulp rounds 4 up.  One lane, and the lanes q, PER + q, ... of one
    group, add in turn; different groups meet in the butterfly.  So the model is order-sensitive where the kernel is,
    and says which order."""
    big, tiny = np.float32(2.0), np.float32(5.0 * 2.0 ** -28)
    s = float(tiny) ** 2
    in_turn, pair_first = (4.0 + s) + s, 4.0 + (s + s)
    assert in_turn == 4.0 and pair_first == 4.0 + 2.0 ** -50
    rows = np.zeros((256, 1), dtype=np.float32)
    rows[0, 0], rows[1, 0], rows[2, 0] = big, tiny, tiny                  # rows 0..2: lane 0, in this order
    assert gm.unit_partial(rows)[0, 0] == in_turn
    rows = np.zeros((256, 1), dtype=np.float32)
    rows[0, 0], rows[8 * 4, 0], rows[16 * 4, 0] = big, tiny, tiny          # lanes 0, 8, 16: group q = 0 (PER = 8 at N = 1)
    assert gm.unit_partial(rows)[0, 0] == in_turn
    rows = np.zeros((256, 1), dtype=np.float32)
    rows[0, 0], rows[1 * 4, 0], rows[9 * 4, 0] = big, tiny, tiny           # lane 0 in group 0; lanes 1 and 9 in group 1
    assert gm.unit_partial(rows)[0, 0] == pair_first


def test_units_chunks_and_second_slot():
    N, D = 7, 3 * 4096 + 1
    xc = _rows(D, N, 811, True)
    slots = gm.unit_slots(xc, UNIT_ROWS)
    assert slots.shape == (4 * gm.PACK, N, N)
    assert np.all(slots[1::2] == 0.0)
    assert np.array_equal(slots[6], np.outer(xc[-1].astype(np.float64), xc[-1].astype(np.float64)))   # the ragged tail
    chunks = gm.reduce_chunks(slots)
    assert chunks.shape == (gm.RC, N, N)
    for u in range(4):           # four units, one per chunk: a chunk is its unit's slot
        assert np.array_equal(chunks[u], slots[2 * u])
    assert np.all(chunks[4:] == 0.0)
    # many units per chunk: 40 units -> 3 per chunk, the last chunks empty
    many = gm.unit_slots(_rows(40 * 1024, 3, 812, True), 1024)
    ch = gm.reduce_chunks(many)
    assert np.all(ch[14:] == 0.0) and np.any(ch[13] != 0.0)
    want, bound = gm.gram_reference(_rows(40 * 1024, 3, 812, True))
    assert np.all(np.abs(gm.gram_total(ch) - want) <= bound)


def test_dropped_or_doubled_row_shows():
    """The spikes: without one block's spike row, or with it twice, some entry is off by far more than the bound."""
    N, D = 8, 4097
    xc = _rows(D, N, 813, False)
    want, bound = gm.gram_reference(xc)
    spike_rows = [b * 256 + (37 * b + 11 * (b % N)) % 256 for b in range(17)]
    for r in spike_rows[:16]:
        dropped = np.delete(xc, r, axis=0)
        doubled = np.insert(xc, r, xc[r], axis=0)
        for other in (dropped, doubled):
            got = gm.gram_total(gm.gram_chunks(other, UNIT_ROWS))
            assert np.any(np.abs(got - want) > 1e6 * bound), r


def test_minus_base_and_half_inputs_are_rows_like_any_other():
    N, D = 4, 1027
    deltas = [d.numpy() for d in orc.synthetic_deltas(D, N, 814, rank=3)]
    base = orc.synthetic_deltas(D, 1, 815, rank=1)[0].numpy()
    ft = [d + base for d in deltas]
    xc = gm.centre(ft, True, base=base)
    assert np.array_equal(xc, gm.centre([f - base for f in ft], True))
    got = gm.gram_total(gm.gram_chunks(xc, 1024))
    want, bound = gm.gram_reference(xc)
    assert np.all(np.abs(got - want) <= bound)
