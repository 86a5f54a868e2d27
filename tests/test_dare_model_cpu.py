"""
The numpy model of the DARE merge (tests/dare_model.py): the generator against the known answers of Philox4x32-10 and a
plain-integer restatement, the threshold rule, the statistics of the mask at a fixed seed, and the places the definition
is sharp -- drop rate 0 is the sequential fp32 sum, seeds and quads give different masks, dropped values are skipped.
"""
import math

import numpy as np
import pytest

import dare_model as dm

KATS = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_int(counter, key):
    """Philox4x32-10 on Python integers, written from the paper's round function."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


@pytest.mark.parametrize("counter,key,want", KATS)
def test_known_answers(counter, key, want):
    assert _philox_int(counter, key) == want
    got = dm.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want


def test_vectorised_generator_equals_the_integer_one():
    g = np.random.default_rng(1)
    ctr = g.integers(0, 2 ** 32, size=(4, 257), dtype=np.uint64)
    key = (0x12345678, 0x9abcdef0)
    got = dm.philox4x32_10(tuple(ctr), key)
    for i in range(ctr.shape[1]):
        assert tuple(int(x) for x in got[:, i]) == _philox_int([int(x) for x in ctr[:, i]], key)
    # words(): counter (G lo, G hi, g >> 2, 0), word g & 3, key (seed lo, seed hi) -- also past 2^32 rows
    seed, row0 = 0xfedcba9876543210, 2 ** 32 - 2
    w = dm.words(9, 5, seed, row0)
    for g_ in range(9):
        for d in range(5):
            G = row0 + d
            blk = _philox_int((G & 0xffffffff, G >> 32, g_ >> 2, 0), (seed & 0xffffffff, seed >> 32))
            assert int(w[g_, d]) == blk[g_ & 3]


def test_threshold_rule():
    assert dm.drop_threshold(0.0) == 0
    assert dm.drop_threshold(0.5) == 2 ** 31
    assert dm.drop_threshold(0.9) == int(0.9 * 2.0 ** 32) == 3865470566
    p = 1.0 - 2.0 ** -33
    # 2^32 - 0.5 in double (a product with a power of two is exact): the largest threshold, 2^32 - 1, and no more
    assert p < 1.0 and dm.drop_threshold(p) == 2 ** 32 - 1
    assert dm.drop_threshold(math.nextafter(1.0, 0.0)) == 2 ** 32 - 1
    assert dm.keep_scale(0.9) == np.float32(1.0 - 0.9) and dm.keep_scale(0.0) == np.float32(1.0)
    assert dm.keep_scale(p) == np.float32(2.0 ** -33)
    # dropped iff word < thr: thr 0 drops nothing, whatever the words are
    assert dm.keep_mask(8, 1000, 0.0, seed=5).all()
    w = dm.words(8, 1000, 5)
    assert np.array_equal(dm.keep_mask(8, 1000, 0.5, seed=5), w >= 2 ** 31)


@pytest.mark.parametrize("p", [0.5, 0.9, 0.99])
def test_kept_counts_lie_within_six_standard_deviations(p):
    D, T = 1 << 20, 8
    kept = dm.keep_mask(T, D, p, seed=0).sum(axis=1)
    mean, sd = D * (1.0 - p), math.sqrt(D * p * (1.0 - p))
    print(p, kept.tolist(), mean, sd)
    assert (np.abs(kept - mean) <= 6 * sd).all(), (kept, mean, sd)      # a fixed outcome: the seed is fixed


def test_drop_rate_zero_with_unit_weights_is_the_sequential_sum():
    g = np.random.default_rng(2)
    v = g.standard_normal((5, 3001)).astype(np.float32)
    out, st = dm.dare_merge(v, drop_rate=0.0)
    s = np.zeros(3001, dtype=np.float32)
    for t in range(5):
        s = (s + v[t]).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), s.view(np.uint32))
    assert st["kept"].tolist() == [3001] * 5 and st["drop_threshold"] == 0 and st["rows"] == 3001
    # weights, normalised in double; scaling and base: one product, one sum
    w = [0.5, 1.5, 2.0, 0.25, 0.75]
    base = g.standard_normal(3001).astype(np.float32)
    out, _ = dm.dare_merge(v, drop_rate=0.0, weights=w, normalize=True, scaling=0.3, base=base)
    w32 = (np.asarray(w) / 5.0).astype(np.float32)
    s = np.zeros(3001, dtype=np.float32)
    for t in range(5):
        s = (s + (w32[t] * v[t]).astype(np.float32)).astype(np.float32)
    want = (base + (np.float32(0.3) * s).astype(np.float32)).astype(np.float32)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_dropped_and_lacking_values_are_skipped_and_survivors_rescaled():
    v = np.array([[1, 2, 3, 4], [10, 20, 30, 40], [100, 200, 300, 400]], dtype=np.float32)
    keep = dm.keep_mask(3, 4, 0.5, seed=11)
    assert keep.any() and not keep.all()      # the case does drop and does keep
    has = np.ones((3, 4), dtype=bool)
    has[1, :2] = False
    out, st = dm.dare_merge(v, has, drop_rate=0.5, seed=11)
    want = ((v / np.float32(0.5)) * (keep & has)).sum(axis=0).astype(np.float32)      # small integers: exact in any order
    assert np.array_equal(out, want)
    assert st["kept"].tolist() == (keep & has).sum(axis=1).tolist()
    out2, _ = dm.dare_merge(v, has, drop_rate=0.5, seed=11, rescale=False)
    assert np.array_equal(out2, (v * (keep & has)).sum(axis=0).astype(np.float32))


def test_seeds_rows_and_quads_give_different_masks():
    a, b = dm.keep_mask(8, 4096, 0.5, seed=0), dm.keep_mask(8, 4096, 0.5, seed=1)
    assert (a != b).mean() > 0.4
    hi = dm.keep_mask(8, 4096, 0.5, seed=1 << 32)      # the upper half of the seed is the second key word
    assert (a != hi).mean() > 0.4
    # tasks 3 and 4 of one row come from different counters: word 3 of quad 0 and word 0 of quad 1
    w = dm.words(8, 64, 7)
    for d in (0, 63):
        q0 = _philox_int((d, 0, 0, 0), (7, 0))
        q1 = _philox_int((d, 0, 1, 0), (7, 0))
        assert q0 != q1 and int(w[3, d]) == q0[3] and int(w[4, d]) == q1[0]
    # a row's words depend on its GLOBAL index: the same parameter further down the store draws another mask
    assert (dm.keep_mask(4, 4096, 0.5, 0, row0=0) != dm.keep_mask(4, 4096, 0.5, 0, row0=4096)).mean() > 0.4
    assert np.array_equal(dm.words(4, 10, 3, row0=5), dm.words(4, 15, 3)[:, 5:])
