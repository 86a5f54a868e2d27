"""
numpy model of the register form of pass 1 (csrc/svdq_gram.hip, 1 <= N <= 8, exact products), sum by sum:

  * lane l of the unit's wavefront owns rows 4l .. 4l+3 of every 256-row block;
  * the row mean over the N tasks is an fp32 sum in task order and one fp32 divide, the centred value an fp32 subtract;
  * a product of two fp32 values is exact in fp64, so v_fma_f64 adds exact products: one rounding per addition;
  * a lane adds the rows 4l + e (e = 0..3) of block 0, then of block 1, ... of its unit to ONE running sum per entry;
  * the 64 lane sums of an entry meet in a fixed order: PER = 64 / (2 NTP) lanes share an entry, lane q of them adds the
    sums of lanes q, PER + q, 2 PER + q, ... in turn, the PER partial sums meet in a butterfly (lane ^ 1, ^ 2, ^ 4);
  * the unit's first partial slot takes the sum, its second slot is zeros;
  * k_reduce (csrc/svdq_small.hip) sums a parameter's slots into SVDQ_RC chunks: four groups take every fourth slot
    into eight interleaved accumulators each, a fixed tree over the eight, the four group sums in group order;
  * the eigen stage (csrc/svdq_eig.h) adds the SVDQ_RC chunks in order.

Everything here is a function of the centred fp32 rows alone, so gather, walk, minus-base and half-precision inputs
are modelled by handing in the rows those routes see.
"""
import numpy as np

BLK = 256       # SVDQ_BLK_ROWS
RC = 16         # SVDQ_RC
PACK = 2        # partial slots per unit at N <= 8
LANES = 64


def ntp_of(N):
    """Task slots of the kernel an N-task plan runs."""
    assert 1 <= N <= 8
    return 4 if N <= 4 else 8


def spiked_deltas(deltas, scale=0.25):
    """``deltas`` (N fp32 arrays of one length) plus one task-dependent spike per 256-row block: block b gets
    scale * (1 + t) at row (37 b + 11 t) % 256 of task t = b % N, so a dropped, doubled or misplaced row moves the Gram
    far beyond rounding."""
    N = len(deltas)
    out = [np.array(d, dtype=np.float32, copy=True) for d in deltas]
    D = out[0].shape[0]
    for b in range((D + BLK - 1) // BLK):
        t = b % N
        r = b * BLK + (37 * b + 11 * t) % BLK
        if r < D:
            out[t][r] += np.float32(scale * (1 + t))
    return out


def centre(deltas, center, base=None):
    """[D, N] fp32: the rows as the kernel centres them (``base``: subtracted first, in fp32, as in minus-base mode)."""
    N = len(deltas)
    v = [np.asarray(d, dtype=np.float32) for d in deltas]
    if base is not None:
        b = np.asarray(base, dtype=np.float32)
        v = [x - b for x in v]
    if center:
        s = np.zeros_like(v[0])
        for x in v:
            s = s + x
        mean = s / np.float32(N)
    else:
        mean = np.zeros_like(v[0])
    return np.stack([x - mean for x in v], axis=1).astype(np.float32)


def unit_partial(xc):
    """[N, N] fp64: what one wavefront leaves in its unit's first slot for the centred rows ``xc`` [n, N] of the unit."""
    n, N = xc.shape
    nblk = max((n + BLK - 1) // BLK, 0)
    pad = np.zeros((nblk * BLK, N), dtype=np.float64)
    pad[:n] = xc                                                 # fp32 -> fp64 is exact
    # [step, lane, task]: step = 4 * block + e is the order in which a lane meets its rows
    seq = pad.reshape(nblk, LANES, 4, N).transpose(0, 2, 1, 3).reshape(nblk * 4, LANES, N)
    acc = np.zeros((LANES, N, N), dtype=np.float64)
    for s in range(seq.shape[0]):
        acc = acc + seq[s][:, :, None] * seq[s][:, None, :]      # exact product, one rounding in the addition
    R = 2 * ntp_of(N)
    PER = LANES // R
    part = acc[0:PER].copy()                                     # lane q of the entry's group starts with lane q
    for k in range(1, R):
        part = part + acc[k * PER:(k + 1) * PER]
    off = 1
    while off < PER:
        part = part + part[np.arange(PER) ^ off]
        off <<= 1
    assert all(np.array_equal(part[0], part[q]) for q in range(PER))
    return part[0]


def unit_slots(xc, unit_rows, plan_rows=None):
    """[units * PACK, N, N] fp64: the partial slots of one parameter (second slot of every unit: zeros).  ``plan_rows``:
    the row count the plan was made for, where the run has fewer (masked routes): its units beyond the rows are zeros."""
    D, N = xc.shape
    units = ((D if plan_rows is None else plan_rows) + unit_rows - 1) // unit_rows
    slots = np.zeros((units * PACK, N, N), dtype=np.float64)
    for u in range(units):
        slots[u * PACK] = unit_partial(xc[u * unit_rows:(u + 1) * unit_rows])
    return slots


def reduce_chunks(slots):
    """[RC, N, N] fp64: k_reduce over one parameter's slots (G = 4 groups, the width of N * N <= 64 entries)."""
    units = slots.shape[0] // PACK
    out = np.zeros((RC,) + slots.shape[1:], dtype=np.float64)
    per = (units + RC - 1) // RC
    G = 4
    for c in range(RC):
        ua = c * per
        ub = min(ua + per, units)
        ua = min(ua, ub)
        a, b = ua * PACK, ub * PACK
        red = []
        for g in range(G):
            acc = [np.zeros(slots.shape[1:], dtype=np.float64) for _ in range(8)]
            s = a + g
            while s + 7 * G < b:
                for u in range(8):
                    acc[u] = acc[u] + slots[s + u * G]
                s += 8 * G
            while s < b:
                acc[0] = acc[0] + slots[s]
                s += G
            red.append(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])))
        t = red[0]
        for g in range(1, G):
            t = t + red[g]
        out[c] = t
    return out


def gram_chunks(xc, unit_rows, plan_rows=None):
    """The SVDQ_RC level-2 partials of one parameter, as k_reduce leaves them in the workspace."""
    return reduce_chunks(unit_slots(xc, unit_rows, plan_rows))


def gram_total(chunks):
    """The Gram the eigen stage solves: the chunks added in order, from zero."""
    a = np.zeros(chunks.shape[1:], dtype=np.float64)
    for c in range(chunks.shape[0]):
        a = a + chunks[c]
    return a


def gram_reference(xc):
    """(G, bound): fp64 numpy Gram of the same centred fp32 rows and the forward-error bound of ANY order of an fp64 sum
    of D exactly known terms, (D - 1) 2^-53 sum |x_i x_j| per entry (Higham, Accuracy and Stability, (4.4), first order
    in u; the terms are exact because fp32 products are)."""
    x = xc.astype(np.float64)
    D = x.shape[0]
    G = x.T @ x
    bound = max(D - 1, 0) * 2.0 ** -53 * (np.abs(x).T @ np.abs(x))
    return G, bound


def workspace_gram2_offset(n_slots, n_params, N):
    """Byte offset of the level-2 Gram partials in a plan's workspace (svdq_plan_create in csrc/svdq_api.hip): unit
    partials of the Gram and of the projection, W, c0, then the chunks."""
    al = lambda x: (x + 255) // 256 * 256
    nn = N * N
    return 2 * al(n_slots * nn * 8) + al(n_params * (nn + 4) * 4) + al(n_params * nn * 8)
