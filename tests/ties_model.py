"""
The numpy model of the sign-elected (TIES) merge as DESIGN.md section 26 defines it -- the truth of the GPU tests, and
itself checked against a torch restatement of the published steps in tests/test_ties_model_cpu.py.

    v      float32 [T, D]: task t's value at row d (0 where the task lacks the parameter), tasks in sorted-name order
    trim   tau_t = the j-th smallest |v_t[.]|, j = max(D - int(D * density), 1); kept iff |v_t[d]| >= tau_t
    elect  s[d] = the kept values added task by task in fp32; positive iff s[d] >= 0
    merge  a[d] = the kept values whose sign strictly agrees, added task by task in fp32; c[d] their number
           mean: a / max(c, 1), sum: a
    apply  base + scaling * merged (one product, one sum, each rounded to fp32)

Every sum is an explicit task-by-task loop over float32 arrays: numpy's own reductions add pairwise.
"""
import numpy as np


def stack_values(per_task, tasks, names, sizes) -> np.ndarray:
    """float32 [T, D] from {task: {param: tensor or array}} (what reconstruct_task_vectors returns): the parameters in
    the order of ``names`` one after the other, zeros where a task lacks a parameter; ``sizes`` {param: elements}."""
    v = np.zeros((len(tasks), sum(int(sizes[n]) for n in names)), dtype=np.float32)
    off = 0
    for n in names:
        for g, t in enumerate(tasks):
            x = per_task.get(t, {}).get(n)
            if x is not None:
                x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
                v[g, off:off + int(sizes[n])] = x.reshape(-1)
        off += int(sizes[n])
    return v


def split_rows(flat: np.ndarray, names, sizes):
    """{param: its slice of a [D] array laid out as ``stack_values`` lays the rows out}."""
    out, off = {}, 0
    for n in names:
        out[n] = flat[off:off + int(sizes[n])]
        off += int(sizes[n])
    return out


def rank_of(D: int, density: float) -> int:
    """j of "the j-th smallest magnitude"."""
    return max(D - int(D * density), 1)


def thresholds(v: np.ndarray, density: float) -> np.ndarray:
    """tau [T] float32."""
    v = np.asarray(v, dtype=np.float32)
    j = rank_of(v.shape[1], density)
    return np.array([np.partition(np.abs(row), j - 1)[j - 1] for row in v], dtype=np.float32)


def ties_merge(v: np.ndarray, density: float, merge_func: str = "mean", scaling: float = 1.0, base=None, tau=None):
    """(out float32 [D], stats).  ``tau``: None = ``thresholds(v, density)``; or thresholds of the caller's own, [T] or
    anything that broadcasts against [T, D] (a test that wants to show what another threshold rule would give).
    stats: thresholds, kept [T], sign_conflict_rows, empty_rows, rows."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    if tau is None:
        tau = thresholds(v, density)
    tau = np.asarray(tau, dtype=np.float32)
    kept = np.abs(v) >= (tau[:, None] if tau.ndim == 1 else tau)
    s = np.zeros(D, dtype=np.float32)
    for t in range(T):
        s = np.where(kept[t], (s + v[t]).astype(np.float32), s)
    positive = s >= 0
    a = np.zeros(D, dtype=np.float32)
    c = np.zeros(D, dtype=np.float32)
    for t in range(T):
        agree = kept[t] & np.where(positive, v[t] > 0, v[t] < 0)
        a = np.where(agree, (a + v[t]).astype(np.float32), a)
        c = np.where(agree, c + np.float32(1), c).astype(np.float32)
    if merge_func == "mean":
        merged = (a / np.maximum(c, np.float32(1))).astype(np.float32)
    elif merge_func == "sum":
        merged = a
    else:
        raise ValueError(merge_func)
    out = (np.float32(scaling) * merged).astype(np.float32)
    if base is not None:
        out = (np.asarray(base, dtype=np.float32) + out).astype(np.float32)
    has_pos, has_neg = (kept & (v > 0)).any(axis=0), (kept & (v < 0)).any(axis=0)
    stats = {"thresholds": tau, "kept": kept.sum(axis=1).astype(np.int64),
             "sign_conflict_rows": int((has_pos & has_neg).sum()), "empty_rows": int((~kept.any(axis=0)).sum()), "rows": D}
    return out, stats
