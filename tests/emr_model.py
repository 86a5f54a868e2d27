"""
The numpy model of the EMR merge (Huang et al. 2024) as DESIGN.md section 31 and include/svdq.h (at svdq_plan_emr_elect)
define it -- the truth of the GPU tests; tests/test_emr_model_cpu.py checks it by hand.

    v, has  float32 / bool [T, D]: task g's value at row d and whether the task has the row's parameter; tasks in
            sorted-name order (store task index g), rows in the caller's order
    sum     S = +0; for the tasks that have the row, in ascending g: S = fl(S + v_g)      (tall_model.task_sum)
    elect   gamma = sign(S) in {+1, 0, -1}; eps = max |v_g| over the tasks that have the row and agree (v_g > 0 for
            gamma = +1, v_g < 0 for gamma = -1), 0 with gamma = 0; tau_uni = +0 with gamma = 0, else copysign(eps, gamma)
    mask    M_g = has_g && v_g * gamma > 0
    rescale A_g = sum |v_g| over the rows the task has, B_g = sum M_g eps, exact sums of float64 terms (math.fsum);
            lambda_g = A_g / B_g, 1.0 where B_g == 0
    apply   out = fl(base + fl(lambda32 * (M_g ? tau_uni : +0))); without base the product
    streams tall_model.pack_streams

Every per-row reduction is an explicit task-by-task loop over float32 arrays: numpy's own reductions add pairwise.
"""
import math

import numpy as np

from tall_model import pack_streams, stack_values, task_sum      # noqa: F401  (imported, not copied)


def elect(v, has=None):
    """(tau_uni float32 [D], masks bool [T, D], eps float32 [D], gamma int8 [D])."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    has = np.ones((T, D), dtype=bool) if has is None else np.asarray(has, dtype=bool)
    s = task_sum(v, has)
    gamma = np.zeros(D, dtype=np.int8)
    gamma[s > 0] = 1
    gamma[s < 0] = -1
    masks = np.zeros((T, D), dtype=bool)
    eps = np.zeros(D, dtype=np.float32)
    for g in range(T):
        masks[g] = has[g] & (((gamma > 0) & (v[g] > 0)) | ((gamma < 0) & (v[g] < 0)))
        eps = np.where(masks[g], np.maximum(eps, np.abs(v[g])), eps).astype(np.float32)
    # fp32 addition is monotone: S > 0 needs some v_g > 0
    assert (eps[gamma != 0] > 0).all(), "eps must be positive wherever a sign is elected"
    assert not eps[gamma == 0].any()
    tau = np.where(gamma == 0, np.float32(0.0), np.copysign(eps, gamma.astype(np.float32))).astype(np.float32)
    return tau, masks, eps, gamma


def sums(v, has, masks, eps):
    """(A float64 [T], B float64 [T]): the exact sums, rounded once."""
    v = np.asarray(v, dtype=np.float32)
    T = v.shape[0]
    has = np.ones(v.shape, dtype=bool) if has is None else np.asarray(has, dtype=bool)
    A = np.array([math.fsum(np.abs(v[g][has[g]]).astype(np.float64).tolist()) for g in range(T)], dtype=np.float64)
    B = np.array([math.fsum(eps[masks[g]].astype(np.float64).tolist()) for g in range(T)], dtype=np.float64)
    return A, B


def rescalers(A, B):
    """float64 [T]: A / B, 1.0 where B == 0."""
    return np.array([a / b if b != 0.0 else 1.0 for a, b in zip(A.tolist(), B.tolist())], dtype=np.float64)


def emr_merge(v, has=None):
    """{"tau", "masks", "eps", "gamma", "A", "B", "lambda"} of T tasks."""
    tau, masks, eps, gamma = elect(v, has)
    A, B = sums(v, has, masks, eps)
    return {"tau": tau, "masks": masks, "eps": eps, "gamma": gamma, "A": A, "B": B, "lambda": rescalers(A, B)}


def task_model(tau, mask, lam, base=None):
    """float32 [D]: fl(base + fl(float32(lam) * (mask ? tau : +0)))."""
    with np.errstate(over="ignore"):
        lam32 = np.float32(lam)
    if not np.isfinite(lam32):
        raise ValueError(f"the rescaler must be finite in fp32, got {lam!r}")
    picked = np.where(np.asarray(mask, dtype=bool), np.asarray(tau, dtype=np.float32), np.float32(0.0)).astype(np.float32)
    out = (lam32 * picked).astype(np.float32)
    if base is not None:
        out = (np.asarray(base, dtype=np.float32) + out).astype(np.float32)
    return out
