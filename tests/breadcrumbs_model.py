"""
The numpy model of the Model Breadcrumbs merge as DESIGN.md section 35 and include/svdq.h define it -- the truth of the
GPU tests, and itself checked against a torch restatement (sort per tensor, keep an index range) in
tests/test_breadcrumbs_model_cpu.py.

    v        float32 [T, D]: task t's value at row d, tasks in sorted-name order, the parameters one after the other
    bounds   [P + 1] row boundaries: parameter p is rows bounds[p] .. bounds[p + 1] - 1, D_p = their number
    present  bool [P][T]: task t has parameter p (what v holds elsewhere is ignored: no implicit zeros)
    counts   n_keep = int(D_p * density), n_top = int(D_p * gamma), n_bot = D_p - n_keep - n_top; n_bot < 0: n_top += n_bot,
             n_bot = 0
    band     n_keep == 0: nothing kept.  Else lo = the (n_bot + 1)-th smallest |v_t| of the tensor, hi = the
             (D_p - n_top)-th; kept iff lo <= |v| <= hi
    combine  without election: a = the kept values added task by task in fp32, c their number.  With: s = that sum,
             positive iff s >= 0; a, c over the kept values whose sign strictly agrees.  sum: a, mean: a / max(c, 1)
    apply    base + scaling * merged (one product, one sum, each rounded to fp32)

Every sum is an explicit task-by-task loop over float32 arrays: numpy's own reductions add pairwise.
"""
import numpy as np


def counts(D: int, density: float, gamma: float):
    """(n_keep, n_top, n_bot): Python integers."""
    D = int(D)
    n_keep, n_top = int(D * density), int(D * gamma)
    n_bot = D - n_keep - n_top
    if n_bot < 0:
        n_top += n_bot
        n_bot = 0
    return n_keep, n_top, n_bot


def band(mag: np.ndarray, density: float, gamma: float):
    """(lo, hi) float32 of one (parameter, task)'s magnitudes, or None where nothing is kept."""
    D = mag.shape[0]
    n_keep, n_top, n_bot = counts(D, density, gamma)
    if n_keep == 0:
        return None
    srt = np.sort(mag)
    return srt[n_bot], srt[D - n_top - 1]


def bands(v, bounds, present, density, gamma):
    """(kept bool [T, D], thresholds [P][T] of (lo, hi) or None): the band of every (parameter, task)."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    P = len(bounds) - 1
    assert bounds[0] == 0 and bounds[-1] == D
    kept = np.zeros((T, D), dtype=bool)
    thresholds = [[None] * T for _ in range(P)]
    for p in range(P):
        a, b = int(bounds[p]), int(bounds[p + 1])
        for t in range(T):
            if not present[p][t] or b == a:
                continue
            mag = np.abs(v[t, a:b])
            lh = band(mag, density, gamma)
            thresholds[p][t] = lh
            if lh is not None:
                kept[t, a:b] = (mag >= lh[0]) & (mag <= lh[1])
    return kept, thresholds


def breadcrumbs_merge(v, bounds, present, density=0.9, gamma=0.01, scaling=1.0, sign_election=False, merge_func="sum",
                      base=None, banded=None):
    """(out float32 [D], stats).  ``banded``: None = ``bands(v, bounds, present, density, gamma)``, or that call's result
    (a test that combines one band several ways).  stats: thresholds [P][T] of (lo, hi) or None (None also where the task
    lacks the parameter), kept int64 [P, T], kept_total [T], sign_conflict_rows, empty_rows, rows."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    P = len(bounds) - 1
    kept, thresholds = bands(v, bounds, present, density, gamma) if banded is None else banded
    a = np.zeros(D, dtype=np.float32)
    c = np.zeros(D, dtype=np.float32)
    if sign_election:
        s = np.zeros(D, dtype=np.float32)
        for t in range(T):
            s = np.where(kept[t], (s + v[t]).astype(np.float32), s)
        positive = s >= 0
    for t in range(T):
        use = kept[t] & np.where(positive, v[t] > 0, v[t] < 0) if sign_election else kept[t]
        a = np.where(use, (a + v[t]).astype(np.float32), a)
        c = np.where(use, c + np.float32(1), c).astype(np.float32)
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
    kept_pt = np.array([[int(kept[t, int(bounds[p]):int(bounds[p + 1])].sum()) for t in range(T)] for p in range(P)],
                       dtype=np.int64).reshape(P, T)
    stats = {"thresholds": thresholds, "kept": kept_pt, "kept_total": kept_pt.sum(axis=0),
             "sign_conflict_rows": int((has_pos & has_neg).sum()), "empty_rows": int((~kept.any(axis=0)).sum()), "rows": D}
    return out, stats
