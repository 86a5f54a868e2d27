"""
The numpy model of the drop-and-rescale (DARE) merge as DESIGN.md section 28 and include/svdq.h (at svdq_plan_dare_merge)
define it -- the truth of the GPU tests; its generator is checked against known answers in tests/test_dare_model_cpu.py.

    v, has  float32 / bool [T, D]: task t's value at global row G and whether the task has the row's parameter; tasks in
            sorted-name order (store task index g), rows in sorted-parameter-name order
    draw    Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (G & 0xffffffff, G >> 32, g >> 2, 0); task g uses
            output word g & 3; thr = min(int(drop_rate * 2**32), 2**32 - 1); dropped iff word < thr
    rescale q = float32(1.0 - drop_rate); a kept value becomes v / q (one fp32 division); rescale=False: v
    combine m = +0; for the kept tasks in ascending g: m = fl(m + fl(w_g * x)); dropped and lacking tasks are skipped
    apply   out = fl(base + fl(scaling * m)); without base the product

Every sum is an explicit task-by-task loop over float32 arrays: numpy's own reductions add pairwise.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Vectorised Philox4x32-10.  counter: four arrays (or integers) of 32-bit words, broadcast against each other; key:
    two integers.  Returns uint32 [4, ...]."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c).astype(np.uint32)


def drop_threshold(drop_rate: float) -> int:
    return min(int(float(drop_rate) * 2.0 ** 32), 2 ** 32 - 1)


def keep_scale(drop_rate: float) -> np.float32:
    return np.float32(1.0 - float(drop_rate))


def words(T: int, D: int, seed: int, row0: int = 0) -> np.ndarray:
    """uint32 [T, D]: the word of (task g, global row row0 + d)."""
    G = np.arange(D, dtype=np.uint64) + np.uint64(row0)
    key = (seed & MASK32, seed >> 32)
    out = np.empty((T, D), dtype=np.uint32)
    for quad in range((T + 3) // 4):
        blk = philox4x32_10((G & np.uint64(MASK32), G >> np.uint64(32), quad, 0), key)
        n = min(4, T - 4 * quad)
        out[4 * quad:4 * quad + n] = blk[:n]
    return out


def keep_mask(T: int, D: int, drop_rate: float, seed: int, row0: int = 0) -> np.ndarray:
    """bool [T, D]: the draw keeps (task g, row).  drop_rate 0 keeps everything (thr = 0)."""
    return words(T, D, seed, row0) >= np.uint32(drop_threshold(drop_rate))


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
    """{param: its slice of a [D] array laid out as ``stack_values`` lays the rows out}."""
    out, off = {}, 0
    for n in names:
        out[n] = flat[off:off + int(sizes[n])]
        off += int(sizes[n])
    return out


def dare_merge(v, has=None, drop_rate=0.9, seed=0, rescale=True, weights=None, normalize=False, scaling=1.0, base=None,
               row0=0, all_words=None):
    """(out float32 [D], stats).  ``weights``: None (1.0 each) or T numbers; ``row0``: the global row of column 0;
    ``all_words``: ``words(T, D, seed, row0)`` of the caller's own (a test that merges one store many times computes
    them once).  stats: kept int64 [T], rows, drop_threshold."""
    v = np.asarray(v, dtype=np.float32)
    T, D = v.shape
    has = np.ones((T, D), dtype=bool) if has is None else np.asarray(has, dtype=bool)
    w = np.ones(T, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    if normalize:
        w = w / float(np.sum(w))
    w = w.astype(np.float32)
    thr = drop_threshold(drop_rate)
    q = keep_scale(drop_rate)
    keep = has.copy()
    if thr:
        if all_words is None:
            all_words = words(T, D, seed, row0)
        keep &= all_words >= np.uint32(thr)
    m = np.zeros(D, dtype=np.float32)
    for t in range(T):
        x = (v[t] / q).astype(np.float32) if rescale else v[t]
        term = (w[t] * x).astype(np.float32)
        m = np.where(keep[t], (m + term).astype(np.float32), m)
    out = (np.float32(scaling) * m).astype(np.float32)
    if base is not None:
        out = (np.asarray(base, dtype=np.float32) + out).astype(np.float32)
    return out, {"kept": keep.sum(axis=1).astype(np.int64), "rows": D, "drop_threshold": thr}
