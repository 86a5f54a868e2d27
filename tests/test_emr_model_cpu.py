"""
tests/emr_model.py checked by hand on tiny arrays: every line of the definition where a choice was
made has a row here whose outcome is written out.
"""
import numpy as np
import pytest

import emr_model as em

F = np.float32


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_a_row_whose_values_cancel_elects_nothing():
    v = np.array([[3.0, 1.0], [-3.0, 2.0], [0.0, -0.5]], dtype=F)      # row 0: 3 - 3 + 0 = 0 with both signs present
    r = em.emr_merge(v)
    assert r["gamma"].tolist() == [0, 1]
    assert _bits(r["tau"])[0] == 0 and not r["masks"][:, 0].any() and r["eps"][0] == 0      # +0, in no mask
    assert r["tau"][1] == F(2.0) and r["masks"][:, 1].tolist() == [True, True, False]
    # row 0 counts in A (|v| of every row the task has) and in no B
    assert r["A"].tolist() == [4.0, 5.0, 0.5] and r["B"].tolist() == [2.0, 2.0, 0.0]
    assert r["lambda"].tolist() == [2.0, 2.5, 1.0]


def test_zeros_of_either_sign_are_in_no_mask():
    v = np.array([[0.0, -0.0, 1.0, -1.0], [-0.0, 0.0, 0.0, -0.0]], dtype=F)
    r = em.emr_merge(v)
    assert r["gamma"].tolist() == [0, 0, 1, -1]
    assert _bits(r["tau"]).tolist() == _bits([0.0, 0.0, 1.0, -1.0]).tolist()      # +0 where nothing is elected
    assert r["masks"].tolist() == [[False, False, True, True], [False, False, False, False]]
    assert r["B"][1] == 0.0 and r["lambda"][1] == 1.0      # B == 0: the decision


def test_one_task_keeps_its_own_vector():
    v = np.array([[1.5, -2.25, 0.0, -0.0, 3e-39, -7.0]], dtype=F)      # a subnormal among them
    r = em.emr_merge(v)
    assert _bits(r["tau"]).tolist() == _bits([1.5, -2.25, 0.0, 0.0, 3e-39, -7.0]).tolist()      # v, with -0 -> +0
    assert r["masks"][0].tolist() == (v[0] != 0).tolist()
    assert r["A"][0] == r["B"][0] and r["lambda"][0] == 1.0
    assert np.array_equal(em.task_model(r["tau"], r["masks"][0], r["lambda"][0]), np.where(v[0] != 0, v[0], F(0)))


def test_a_task_that_lacks_a_parameter():
    v = np.array([[1.0, 1.0, 1.0], [-5.0, -5.0, 2.0], [0.5, 0.5, 0.5]], dtype=F)
    has = np.array([[True, True, True], [False, False, True], [True, True, True]])
    r = em.emr_merge(v, has)
    # rows 0, 1: task 1's -5 is not there: S = 1.5 > 0; its bits are 0 and its A holds row 2 alone
    assert r["gamma"].tolist() == [1, 1, 1] and r["tau"].tolist() == [1.0, 1.0, 2.0]
    assert r["masks"][1].tolist() == [False, False, True]
    assert r["A"].tolist() == [3.0, 2.0, 1.5] and r["B"].tolist() == [4.0, 2.0, 4.0]
    with_it = em.emr_merge(v)
    assert with_it["gamma"].tolist() == [-1, -1, 1] and with_it["tau"].tolist() == [-5.0, -5.0, 2.0]


def test_the_largest_magnitude_of_a_disagreeing_task_is_not_elected():
    v = np.array([[2.0], [3.0], [-4.0]], dtype=F)      # S = 1 > 0; the largest |v| is the negative one
    r = em.emr_merge(v)
    assert r["gamma"].tolist() == [1] and r["tau"].tolist() == [3.0] and r["eps"].tolist() == [3.0]
    assert r["masks"][:, 0].tolist() == [True, True, False]
    assert r["A"].tolist() == [2.0, 3.0, 4.0] and r["B"].tolist() == [3.0, 3.0, 0.0]
    assert r["lambda"].tolist() == [2.0 / 3.0, 1.0, 1.0]


def test_masked_elected_vector_has_the_sign_of_the_task_wherever_set():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((7, 4000)).astype(F)
    v[rng.random(v.shape) < 0.1] = 0.0
    has = rng.random(v.shape) < 0.9
    r = em.emr_merge(v, has)
    for g in range(7):
        picked = np.where(r["masks"][g], r["tau"], F(0))
        assert (np.sign(picked[r["masks"][g]]) == np.sign(v[g][r["masks"][g]])).all()
        assert (np.abs(picked[r["masks"][g]]) >= np.abs(v[g][r["masks"][g]])).all()      # eps is the agreeing maximum
        assert not r["masks"][g][~has[g]].any() and not r["masks"][g][v[g] == 0].any()
    # the paper's mask: v_g * tau_uni > 0 (evaluated in double: no underflow)
    assert np.array_equal(r["masks"], has & (v.astype(np.float64) * r["tau"].astype(np.float64) > 0))
    assert len(set(r["lambda"].tolist())) == 7 and (r["lambda"] > 0).all() and (r["lambda"] < 1).all()


def test_the_sum_is_added_task_by_task_in_fp32():
    # 2^24 + 1 + 1 in fp32: task by task the ones are lost, S = 2^24 - 2^24 = 0 although the exact sum is 2
    v = np.array([[16777216.0], [1.0], [1.0], [-16777216.0]], dtype=F)
    r = em.emr_merge(v)
    assert r["gamma"].tolist() == [0] and not r["masks"].any()
    assert em.emr_merge(v[[1, 2, 0, 3]])["gamma"].tolist() == [1]      # another order: 1 + 1 + 2^24 is exact


def test_task_model_rounds_the_product_then_the_sum():
    tau = np.array([1.0000001, -3.0, 2.0, 0.1], dtype=F)
    mask = np.array([True, False, True, True])
    base = np.array([1e8, 1.0, -2.0, 0.3], dtype=F)
    lam = 0.7
    want = [F(F(base[i]) + F(F(lam) * (tau[i] if mask[i] else F(0)))) for i in range(4)]
    assert _bits(em.task_model(tau, mask, lam, base)).tolist() == _bits(want).tolist()
    assert _bits(em.task_model(tau, mask, -lam)).tolist() == _bits([F(-lam) * tau[0], -0.0, F(-lam) * tau[2],
                                                                    F(-lam) * tau[3]]).tolist()
    with pytest.raises(ValueError):
        em.task_model(tau, mask, float("inf"))
    with pytest.raises(ValueError):
        em.task_model(tau, mask, 1e39)


def test_sums_are_exact():
    v = np.array([[1e8, 1.0, -1.0, 1e-8] * 1000], dtype=F)
    r = em.emr_merge(v)
    import math
    assert r["A"][0] == math.fsum([float(F(1e8)), 1.0, 1.0, float(F(1e-8))] * 1000)
