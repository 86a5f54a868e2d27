"""
The numpy model of TALL masks and the consensus merge as DESIGN.md section 30 and include/svdq.h (at
svdq_plan_tall_consensus) define them -- the truth of the GPU tests; tests/test_tall_model_cpu.py checks it by hand.

    v, has  float32 / bool [T, D]: task t's value at row d and whether the task has the row's parameter; tasks in
            sorted-name order (store task index g), rows in the caller's order
    sum     S = +0; for the tasks that have the row, in ascending g: S = fl(S + v_g)
    mask    R_g = fl(S - v_g); m_g = |v_g| > fl(lambda_g * |R_g|), STRICT; 0 where the task lacks the row
    consensus  c = the set masks of the row; kept iff c >= k; m = kept ? S : +0
    apply   out = fl(base + fl(scaling * m)); without base the product
    streams numpy.packbits order: the bit of row d of parameter p is stream bit bit_base[p] + d; everything else is 0

Every sum is an explicit task-by-task loop over float32 arrays: numpy's own reductions add pairwise.
"""
import numpy as np


def lambdas_of(tall_lambda, T: int) -> np.ndarray:
    """float32 [T] from one number or T numbers."""
    lam = np.asarray(tall_lambda, dtype=np.float64)
    lam = np.full(T, float(lam)) if lam.ndim == 0 else lam
    if lam.shape != (T,) or not np.isfinite(lam).all() or (lam < 0).any():
        raise ValueError(f"tall_lambda must be one finite number >= 0 or {T} of them, got {tall_lambda!r}")
    return lam.astype(np.float32)


def task_sum(v, has=None) -> np.ndarray:
    """S float32 [D]."""
    v = np.asarray(v, dtype=np.float32)
    has = np.ones(v.shape, dtype=bool) if has is None else np.asarray(has, dtype=bool)
    s = np.zeros(v.shape[1], dtype=np.float32)
    for g in range(v.shape[0]):
        s = np.where(has[g], (s + v[g]).astype(np.float32), s)
    return s


def tall_masks(v, has=None, tall_lambda=0.4) -> np.ndarray:
    """bool [T, D]."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    has = np.ones((T, D), dtype=bool) if has is None else np.asarray(has, dtype=bool)
    lam = lambdas_of(tall_lambda, T)
    s = task_sum(v, has)
    m = np.zeros((T, D), dtype=bool)
    for g in range(T):
        rest = (s - v[g]).astype(np.float32)
        bound = (lam[g] * np.abs(rest)).astype(np.float32)
        m[g] = has[g] & (np.abs(v[g]) > bound)
    return m


def consensus_merge(v, has=None, tall_lambda=0.4, k=2, scaling=1.0, base=None):
    """(out float32 [D], masks bool [T, D], stats).  stats: active int64 [T], agreement int64 [T + 1], rows."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= T:
        raise ValueError(f"k must be an integer in [0, {T}], got {k!r}")
    m = tall_masks(v, has, tall_lambda)
    s = task_sum(v, has)
    c = m.sum(axis=0)
    merged = np.where(c >= k, s, np.float32(0.0)).astype(np.float32)
    out = (np.float32(scaling) * merged).astype(np.float32)
    if base is not None:
        out = (np.asarray(base, dtype=np.float32) + out).astype(np.float32)
    stats = {"active": m.sum(axis=1).astype(np.int64), "agreement": np.bincount(c, minlength=T + 1).astype(np.int64),
             "rows": D}
    return out, m, stats


def pack_streams(masks_by_param, bit_base, total_bits: int) -> np.ndarray:
    """uint8 [T, ceil(total_bits / 8)]: ``masks_by_param`` {param: bool [T, rows]} placed at ``bit_base[param]`` of a
    stream of ``total_bits`` zero bits, packed by numpy.packbits."""
    T = next(iter(masks_by_param.values())).shape[0] if masks_by_param else 0
    bits = np.zeros((T, total_bits), dtype=bool)
    for name, m in masks_by_param.items():
        m = np.asarray(m, dtype=bool)
        at = int(bit_base[name])
        if at < 0 or at + m.shape[1] > total_bits:
            raise ValueError(f"{name}: bits [{at}, {at + m.shape[1]}) lie outside the stream of {total_bits} bits")
        bits[:, at:at + m.shape[1]] = m
    return np.packbits(bits, axis=1) if total_bits else np.zeros((T, 0), dtype=np.uint8)


def stack_values(per_task, tasks, names, sizes):
    """(v float32 [T, D], has bool [T, D]) from {task: {param: tensor or array}} (what reconstruct_task_vectors
    returns): the parameters in the order of ``names`` one after the other; ``sizes`` {param: elements}."""
    D = sum(int(sizes[n]) for n in names)
    v = np.zeros((len(tasks), D), dtype=np.float32)
    has = np.zeros((len(tasks), D), dtype=bool)
    off = 0
    for n in names:
        for g, t in enumerate(tasks):
            x = per_task.get(t, {}).get(n)
            if x is not None:
                x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
                v[g, off:off + int(sizes[n])] = x.reshape(-1)
                has[g, off:off + int(sizes[n])] = True
        off += int(sizes[n])
    return v, has


def split_rows(flat: np.ndarray, names, sizes):
    """{param: its slice (of the last axis) of an array laid out as ``stack_values`` lays the rows out}."""
    out, off = {}, 0
    for n in names:
        out[n] = flat[..., off:off + int(sizes[n])]
        off += int(sizes[n])
    return out
