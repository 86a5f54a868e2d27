"""
GPU tests of svdq_plan_consolidate_eig / svdq_plan_rebase (include/svdq.h; CompressPlan.consolidate): a plan's stored
artifacts brought back to the form a fresh compress run of the tasks they reconstruct would give them.

Stores are adopted plans filled by svdq_plan_import from tensors made here (the pattern of tests/test_hip_store_gram.py):
U random and NOT orthonormal, random finite codes / scales / zero points, spikes of 1e3 x the typical magnitude in U and
the mean at the first and last rows of blocks, units and the parameter.  The truth is fp64 numpy on the bytes copied
back from the plans' own buffers.  Every bound is derived where it is used:

  rebase, per element     |out - (A Wt)64| <= (r + 3) 2^-24 sum_i |a_i| |wt_i| + the rounding to the element type
                          (fp16: 2^-11 |x|, 2^-25 below the normal range; fp32: none).  The kernel forms ONE fp32 fma chain
                          of r + 1 terms per element (gamma_{r+1}), W and bbar are read as the fp32 values the test reads.
  eigen stage             |lambda - lambda64| <= c n eps64 ||K||_F + 2 (2 ra + 2) eps64 ||S||_F, c = 64, n = max(N', ra).
                          The first term is the issue's: a Jacobi / LAPACK eigenvalue of the matrix each solver was GIVEN is
                          within a modest multiple of n eps64 ||K|| (Weyl; c = 64 covers both solvers).  The second is
                          what the two solvers were given: K = Bc^T M Bc is formed on the device and here in fp64 from
                          the same M and the same fp32 coefficients, two nested sums of ra terms each, so either copy is
                          within (2 ra + 2) eps64 of S = |Bc|^T |M| |Bc| per entry.  With spiked, sign-mixed data S is much
                          larger than K, which is why it multiplies the formation constant only.
  the property            see test_reconstruction_is_preserved.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import bits_equal

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS64 = 2.0 ** -53
SENT = 0xA5
ROWS = [1, 3, 13, 255, 256, 257, 700, 4097, 127, 128, 129, 513]      # both block sizes' edges: RB = 256 and 128
TASKS = [1, 3, 8, 9, 17, 32]
KINDS = ["k0", "kr", "rlt", "rN"]      # k = 0; k = r; r < N; r = N
UNIT_ROWS = 512
STAGES = 2


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle as o
    o.build_c_oracle()
    return o


def _dev():
    return torch.device("cuda", 0)


def _kr(rows, n, kind):
    r = max(1, n - 2) if kind == "rlt" else n
    r = min(r, rows, n)
    k = {"k0": 0, "kr": r, "rlt": 1, "rN": 1}[kind]
    return min(k, r), r


class Store:
    """A ragged adopted plan: one parameter per entry of ``rows`` (None = a parameter whose rows_dev is 0); entry e has
    the (k, r) kind KINDS[(e + shift) % 4] unless ``made`` gives its tensors."""

    def __init__(self, n, *, fp16, center, rows=ROWS, zero_at=3, shift=0, bits=4, seed=0, made=None):
        from svdq_amd.pipeline import CompressPlan
        dev = _dev()
        rows = list(rows)
        if zero_at is not None:
            rows.insert(zero_at, None)
        g = torch.Generator().manual_seed(7919 * n + 31 * seed + shift)
        self.n, self.fp16, self.center, self.dev = n, fp16, center, dev
        self.rows = [r if r is not None else 0 for r in rows]
        plan_rows = [r if r is not None else 300 for r in rows]
        self.plan_rows = plan_rows
        self.plan = CompressPlan(plan_rows, n, center=center, fp16=fp16, low_bits=bits, rtvq_stages=STAGES, device=dev,
                                 unit_rows=UNIT_ROWS, workspace=False)
        udt = torch.float16 if fp16 else torch.float32
        self.kr, us, means, entries = [], [], [], []
        q = 1 << bits
        for e, rws in enumerate(rows):
            if rws is None:
                self.kr.append((0, 0))
                us.append(None)
                means.append(None)
                entries.append(None)
                continue
            if made is not None:      # (U [rows, r] fp64, mean [rows] or None, C [r, n] fp64): all on the high side
                u64, m64, C = made[e]
                r = k = u64.shape[1]
                u, m = torch.from_numpy(u64).float(), torch.from_numpy(m64 if m64 is not None else np.zeros(rws)).float()
                c_high = np.ascontiguousarray(C.T).astype(np.float16)
                codes = np.zeros((n, STAGES, 0), np.uint8)
                scale = np.ones((n, STAGES), np.float32)
                zp = np.zeros((n, STAGES), np.float32)
            else:
                k, r = _kr(rws, n, KINDS[(e + shift) % 4])
                typ = 1.0 / np.sqrt(rws)
                u = (torch.randn(rws, r, generator=g) + 0.5 * torch.randn(rws, 1, generator=g)) * typ
                m = torch.randn(rws, generator=g) * typ
                # spikes at the first and last rows of every 128-row block (so of 256-row blocks, units and the
                # parameter too), signs at random: enough independent spike rows keep U^T U well conditioned
                edges = sorted({s for b in range(0, rws, 128) for s in (b, b + 127) if s < rws} | {rws - 1})
                for s in edges:
                    sign = torch.where(torch.rand(r, generator=g) < 0.5, -1.0, 1.0)
                    u[s] = 1.0e3 * typ * sign * (1.0 + 0.25 * torch.rand(r, generator=g))
                    m[s] = -1.0e3 * typ
                c_high = torch.randn(n, k, generator=g).numpy().astype(np.float16)
                codes = torch.randint(0, q, (n, STAGES, r - k), generator=g).numpy().astype(np.uint8)
                scale = (2.0 + 30.0 * torch.rand(n, STAGES, generator=g)).numpy().astype(np.float32)
                zp = torch.randint(0, q, (n, STAGES), generator=g).numpy().astype(np.float32)
            self.kr.append((k, r))
            us.append(u.to(udt))
            means.append(m)
            entries.append({"rows": rws, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
                            "c_high": c_high, "codes": codes, "scale": scale, "zero_point": zp,
                            "residual_norm": np.zeros((n, STAGES), np.float32)})
        self.entries, self.us, self.means = entries, us, means
        self.upload()
        self.rows_dev = torch.tensor(self.rows, dtype=torch.int64).to(dev)

    def upload(self):
        from svdq_amd.pipeline import pack_small
        dev, n = self.dev, self.n
        host = pack_small(self.plan.layout, len(self.rows), n, STAGES, self.entries)
        uh = [None if u is None else u[:, :k].contiguous().to(dev) for u, (k, r) in zip(self.us, self.kr)]
        ul = [None if u is None else u[:, k:].contiguous().to(dev) for u, (k, r) in zip(self.us, self.kr)]
        mn = [None if m is None else m.to(dev) for m in self.means] if self.center else None
        self.plan.import_artifacts(uh, ul, mn, host)

    def dst(self, n_dst=None, *, center=True, thr=0.9, max_rank=None, bits=4, stages=STAGES):
        from svdq_amd.pipeline import CompressPlan
        return CompressPlan(self.plan_rows, n_dst or self.n, energy_threshold=thr, max_rank=max_rank, center=center,
                            fp16=self.fp16, low_bits=bits, rtvq_stages=stages, device=self.dev, unit_rows=UNIT_ROWS,
                            workspace=False)


def _source(plan, sm, p, rows, orc):
    """(A [rows, ra], B [ra, N]) in fp64 from the plan's own buffers: what the kernels read."""
    k, r = int(sm.k[p]), int(sm.r[p])
    uh, ul, mean = plan.basis_tensors(p, k, r, rows)
    A = torch.cat([uh, ul], dim=1).double().cpu().numpy()
    n = plan.N
    C = np.zeros((r, n))
    for t in range(n):
        C[:k, t] = sm.c_high[p, t, :k].astype(np.float64)
        if r > k:
            low = orc.rtvq_dequantize({"codes": sm.codes[p, t, :, :r - k].copy(), "scale": sm.scale[p, t].copy(),
                                       "zero_point": sm.zero_point[p, t].copy()})
            C[k:, t] = low.reshape(-1).astype(np.float64)
    if mean is not None:
        A = np.concatenate([A, mean.double().cpu().numpy().reshape(rows, 1)], axis=1)
        C = np.concatenate([C, np.ones((1, n))], axis=0)
    return A, C


def _small_raw(plan):
    """The small views of a plan without fetch_small's NonFiniteInput."""
    from svdq_amd.pipeline import small_views
    return small_views(plan.small.cpu().numpy(), plan.layout, plan.P, plan.N, plan.S)


def _table(src):
    from svdq_amd.pipeline import consolidate_views
    return consolidate_views(src.rebase_table.cpu().numpy(), src.consolidate_layout(), src.P)


def _sentinel(dst):
    dst.basis.fill_(SENT)
    if dst.mean is not None:
        dst.mean.view(torch.uint8).fill_(SENT)


def _half_ulp(x, fp16):
    if not fp16:
        return np.zeros_like(x)
    return np.maximum(2.0 ** -11 * np.abs(x), 2.0 ** -25)


@functools.lru_cache(maxsize=None)
def _run(n, fp16, sc, dc):
    """One consolidation of the ragged store (identity keep), everything the checks need on the host."""
    from oracle import svd_hybrid_oracle as orc
    orc.build_c_oracle()
    shift = TASKS.index(n) + 2 * int(fp16) + int(sc) + 3 * int(dc)
    st = Store(n, fp16=fp16, center=sc, shift=shift)
    dst = st.dst(center=dc)
    _sentinel(dst)
    _, M = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    st.plan.consolidate_eig(dst, list(range(n)), rows_dev=st.rows_dev, basis_gram=M)
    st.plan.rebase(dst, rows_dev=st.rows_dev)
    torch.cuda.synchronize()
    out = {"st": st, "dst": dst, "M": M.cpu().numpy(), "tab": _table(st.plan), "sm": _small_raw(dst),
           "ssm": _small_raw(st.plan), "basis": dst.basis.cpu().numpy().copy(),
           "mean": None if dst.mean is None else dst.mean.view(torch.uint8).cpu().numpy().copy()}
    out["src"] = [None if rws == 0 else _source(st.plan, out["ssm"], p, rws, orc) for p, rws in enumerate(st.rows)]
    return out


SWEEP = [(n, f, sc, dc) for n in TASKS for f in (True, False) for sc in (True, False) for dc in (True, False)]
SWEEP_IDS = [f"n{n}-{'fp16' if f else 'fp32'}-{'c' if sc else 'u'}2{'c' if dc else 'u'}" for n, f, sc, dc in SWEEP]


def _outputs(dst, p, kn, rn, rows):
    uh, ul, mean = dst.basis_tensors(p, kn, rn, rows)
    U = torch.cat([uh, ul], dim=1).double().cpu().numpy()
    return U, (None if mean is None else mean.double().cpu().numpy().reshape(rows))


# ------------------------------------------------------------------------------------------ the streaming pass, row-exact
@pytest.mark.parametrize("n,fp16,sc,dc", SWEEP, ids=SWEEP_IDS)
def test_rebase_rows_against_fp64(sq, n, fp16, sc, dc):
    R = _run(n, fp16, sc, dc)
    st, dst, tab = R["st"], R["dst"], R["tab"]
    es = 2 if fp16 else 4
    touched_b = np.zeros(R["basis"].size, bool)
    touched_m = None if R["mean"] is None else np.zeros(R["mean"].size, bool)
    some = 0
    for p, rws in enumerate(st.rows):
        rn, kn = int(tab.r[p]), int(tab.k[p])
        if rws == 0:
            assert tab.live[p] == 0 and rn == 0 and kn == 0
            continue
        assert tab.live[p] == 1, p
        A, _ = R["src"][p]
        ra = A.shape[1]
        r = st.kr[p][1]
        Wt = tab.w[p, :ra, :rn].astype(np.float64)
        bb = tab.bbar[p, :ra].astype(np.float64)
        U, mean = _outputs(dst, p, kn, rn, rws)
        want = A @ Wt
        bound = (r + 3) * U32 * (np.abs(A) @ np.abs(Wt)) + _half_ulp(want, fp16)
        err = np.abs(U - want)
        assert (err <= bound).all(), (p, rws, float((err / np.maximum(bound, 1e-300)).max()))
        if dc:
            wantm = A @ bb
            boundm = (r + 3) * U32 * (np.abs(A) @ np.abs(bb))
            assert (np.abs(mean - wantm) <= boundm).all(), (p, rws)
            o = 4 * dst.mean_off[p]
            touched_m[o:o + 4 * rws] = True
        o = dst.slab_off[p]
        touched_b[o:o + rws * kn * es] = True
        o += (rws * kn * es + 255) // 256 * 256
        touched_b[o:o + rws * (rn - kn) * es] = True
        some += rn
    assert some > 0 or (n == 1 and dc)      # one centred task: r' = 0 everywhere, only the mean is written
    # nothing outside the three ranges of a parameter: slab gaps, tails and the zero-row entry keep the sentinel
    assert (R["basis"][~touched_b] == SENT).all()
    if touched_m is not None:
        assert (R["mean"][~touched_m] == SENT).all()
    # the same bits in every run
    tab0, small0 = st.plan.rebase_table.clone(), dst.small.clone()
    st.plan.consolidate_eig(dst, list(range(n)), rows_dev=st.rows_dev)
    st.plan.rebase(dst, rows_dev=st.rows_dev)
    torch.cuda.synchronize()
    assert torch.equal(st.plan.rebase_table, tab0) and torch.equal(dst.small, small0)
    assert np.array_equal(dst.basis.cpu().numpy(), R["basis"])
    if R["mean"] is not None:
        assert np.array_equal(dst.mean.view(torch.uint8).cpu().numpy(), R["mean"])


# ------------------------------------------------------------------------------------------ the eigen stage against fp64
def _bc(B, keep, centred):
    Bk = B[:, keep]
    bbar = Bk.sum(axis=1) / len(keep) if centred else np.zeros(B.shape[0])
    return Bk - bbar[:, None], bbar


def _rank_rule(sig32, thr, max_rank):
    """basis.py:147-156, :199-211 in sequential fp32, as the device evaluates it."""
    f = np.float32
    total = f(0)
    for s in sig32:
        total = f(total + f(s * s))
    cum = []
    run = f(0)
    for s in sig32:
        run = f(run + f(s * s))
        cum.append(f(1) if total < f(1e-10) else f(run / total))
    k = 1 + sum(1 for c in cum if c < f(thr))
    if max_rank:
        k = min(k, max_rank)
    k = min(k, len(sig32))
    return k, (float(cum[k - 1]) if k > 0 else 0.0), cum


def _check_eig(R, p, keep, dc, min_sigma=0.0):
    st, tab, sm = R["st"], R["tab"], R["sm"]
    rws = st.rows[p]
    A, B = R["src"][p]
    ra, r = A.shape[1], st.kr[p][1]
    M = R["M"][p][:ra, :ra]
    Bc, bbar = _bc(B, keep, dc)
    nk = len(keep)
    K = Bc.T @ M @ Bc
    S = np.abs(Bc).T @ np.abs(M) @ np.abs(Bc)
    nn = max(nk, ra)
    tol = 64 * nn * EPS64 * np.linalg.norm(K) + 2 * (2 * ra + 2) * EPS64 * np.linalg.norm(S)
    lam = tab.lam[p, :nk]
    lam64 = np.linalg.eigvalsh(K)[::-1]
    assert (np.diff(lam) <= 0).all(), (p, lam)                                  # descending
    assert (np.abs(lam - lam64) <= tol).all(), (p, float(np.abs(lam - lam64).max() / max(tol, 1e-300)))
    assert np.allclose(tab.bbar[p, :ra], bbar.astype(np.float32), rtol=2.0 ** -22, atol=1e-12 * np.abs(B).max())
    # eta: the formula, to fp64 rounding
    g = (np.sqrt(np.maximum(np.diag(M), 0.0))[:, None] * np.abs(Bc)).sum(axis=0)
    eta = (256 + r + 3) * U32 * float((g * g).sum())
    assert abs(tab.eta[p] - eta) <= 1e-12 * eta, (p, tab.eta[p], eta)
    # the keep rule, exactly, from the device's lambda and eta
    floor_ = max(4.0 * tab.eta[p], min_sigma * min_sigma * lam[0])
    rn = 0
    while rn < min(nk, rws) and lam[rn] > floor_ and lam[rn] > 0.0:
        rn += 1
    assert int(tab.r[p]) == rn == int(sm.r[p]), (p, tab.r[p], rn)
    assert abs(tab.dropped[p] - np.clip(lam[rn:], 0, None).sum()) <= 1e-12 * max(tab.dropped[p], 1e-300)
    sig = sm.sigma[p]
    assert np.allclose(sig[:rn], np.sqrt(lam[:rn]).astype(np.float32), rtol=2.0 ** -23, atol=0)
    assert not sig[rn:].any()
    assert int(sm.rows[p]) == rws
    # eigenvectors: V[j][i] = coef[slot j][i] / sigma_i carries the fp32 rounding of coef and sigma (2^-22 relative),
    # so ||K v - lambda v|| <= tol + 2^-22 (||K|| + |lambda|) ||v||; sign: the largest-magnitude component positive
    coef = sm.coef[p].astype(np.float64)
    for i in range(rn):
        v = coef[keep_slots(R, p, nk), i] / float(sig[i])
        res = np.linalg.norm(K @ v - lam[i] * v)
        assert res <= tol + 2.0 ** -21 * (np.linalg.norm(K, 2) + abs(lam[i])) * np.linalg.norm(v), (p, i, res)
        assert abs(np.linalg.norm(v) - 1.0) < 1e-5
        assert v.max() >= -v.min() * (1 - 1e-5), (p, i)      # near-ties of magnitude apart, in fp32
    return rn


def keep_slots(R, p, nk):
    return R.get("slots", list(range(nk)))


@pytest.mark.parametrize("n,fp16,sc,dc", SWEEP, ids=SWEEP_IDS)
def test_eigen_stage_against_fp64(sq, orc, n, fp16, sc, dc):
    R = _run(n, fp16, sc, dc)
    st, sm = R["st"], R["sm"]
    for p, rws in enumerate(st.rows):
        if rws == 0:
            for f in ("sigma", "k", "r", "energy", "rows", "c_high", "codes", "scale", "zero_point", "residual_norm", "coef"):
                assert not getattr(sm, f)[p].any(), (p, f)
            continue
        rn = _check_eig(R, p, list(range(n)), dc)
        kn, en, cum = _rank_rule(sm.sigma[p, :rn], 0.9, None)
        assert int(sm.k[p]) == kn == int(R["tab"].k[p]) and float(sm.energy[p]) == np.float32(en), (p, kn, en)
        _check_tail(sm, p, n, kn, rn, 4, STAGES, orc)


def _check_tail(sm, p, n, kn, rn, bits, stages, orc, slots=None):
    """compress_single_task's tail on the device's coef: c_high = fp16(coef[:k']), codes / scale / zero point = the C
    model's quantizer on coef[k':r'], bit for bit; absent slots are zeros."""
    slots = list(range(n)) if slots is None else slots
    for t in range(n):
        c = sm.coef[p, t]
        if t not in slots:
            assert not c.any() and not sm.c_high[p, t].any() and not sm.codes[p, t].any()
            assert not sm.scale[p, t].any() and not sm.zero_point[p, t].any()
            continue
        assert not c[rn:].any()
        assert np.array_equal(sm.c_high[p, t, :kn].view(np.uint16), c[:kn].astype(np.float16).view(np.uint16))
        assert not sm.c_high[p, t, kn:].any()
        if rn > kn:
            want = orc.rtvq_quantize(c[kn:rn].copy(), bits, stages)
            assert np.array_equal(sm.codes[p, t, :, :rn - kn], want["codes"]), (p, t)
            assert bits_equal(sm.scale[p, t], want["scale"]), (p, t)      # NaN == NaN: a one-element c_low has no range
            assert bits_equal(sm.zero_point[p, t], want["zero_point"]), (p, t)
        assert not sm.codes[p, t, :, max(rn - kn, 0):].any()


@functools.lru_cache(maxsize=None)
def _small_store():
    st = Store(8, fp16=True, center=True, rows=[13, 257, 700], zero_at=None, shift=3)
    _, M = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    return st, M


@pytest.mark.parametrize("max_rank", [None, 1])
@pytest.mark.parametrize("thr", [0.5, 0.9, 0.95, 1.0])
def test_rank_rule_at_thresholds(sq, orc, thr, max_rank):
    st, M = _small_store()
    dst = st.dst(thr=thr, max_rank=max_rank)
    st.plan.consolidate_eig(dst, list(range(8)), rows_dev=st.rows_dev, basis_gram=M)
    sm = _small_raw(dst)
    for p in range(len(st.rows)):
        rn = int(sm.r[p])
        assert rn >= 2
        kn, en, cum = _rank_rule(sm.sigma[p, :rn], thr, max_rank)
        assert int(sm.k[p]) == kn and float(sm.energy[p]) == np.float32(en), (p, thr, max_rank)
        S = torch.from_numpy(sm.sigma[p, :rn].copy())
        # torch's cumsum and the in-order fp32 sums differ by at most (2 n + 1) 2^-24 of a value <= 1
        ulp = (2 * rn + 1) * U32
        if all(abs(float(c) - np.float32(thr)) > ulp for c in cum):      # the rule does not hang on that
            assert kn == orc.select_rank(S, thr, max_rank)
        assert abs(en - float(orc.energy_spectrum(S)[kn - 1])) <= ulp


@pytest.mark.parametrize("stages", [1, 3])
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_quantizer_tail_bit_for_bit(sq, orc, bits, stages):
    st, M = _small_store()
    dst = st.dst(thr=0.5, bits=bits, stages=stages)
    st.plan.consolidate_eig(dst, list(range(8)), rows_dev=st.rows_dev, basis_gram=M)
    sm = _small_raw(dst)
    widest = 0
    for p in range(len(st.rows)):
        rn, kn = int(sm.r[p]), int(sm.k[p])
        widest = max(widest, rn - kn)
        _check_tail(sm, p, 8, kn, rn, bits, stages, orc)
    assert widest >= 3      # a c_low of several elements went through the quantizer


# ------------------------------------------------------------------------------------------ the property that matters
def _dequantized(sm, p, t, kn, rn, orc):
    c = np.zeros(rn)
    c[:kn] = sm.c_high[p, t, :kn].astype(np.float64)
    if rn > kn:
        c[kn:] = orc.rtvq_dequantize({"codes": sm.codes[p, t, :, :rn - kn].copy(), "scale": sm.scale[p, t].copy(),
                                      "zero_point": sm.zero_point[p, t].copy()}).astype(np.float64)
    return c


def _check_property(R, p, keep, slots, fp16, dc, orc):
    """For kept task j (source slot keep[j], destination slot slots[j]): U' c' + mean' from the ROUNDED outputs and the
    fp32 coef against the source's A b_j, both from the bytes the device holds.
      U' = rd(A W) with W the fp32 table: per element |u' - (A W)| <= chain + rounding, chain = (r + 3) 2^-24 |a| |W|,
      rounding <= 2^-11 |u'| (1 + 2^-10) (fp16; 2^-25 below the normal range; fp32: 0); mean' likewise without rounding.
      So |U' c' + mean' - A (W c' + bbar)| <= sum_i (rounding_i + chain_i) |c'_i| + chain_mean   elementwise,
      and A (W c' + bbar) - A b_j is the dropped part plus what the fp32 roundings of W, bbar and c' (2^-24 relative each,
      inside the (r + 3) of the chain term: r + 1 chain steps and two roundings) leave: in norm <= sqrt(dropped + eta)."""
    st, dst, tab, sm = R["st"], R["dst"], R["tab"], R["sm"]
    rws = st.rows[p]
    A, B = R["src"][p]
    ra, r = A.shape[1], st.kr[p][1]
    rn, kn = int(tab.r[p]), int(tab.k[p])
    U, mean = _outputs(dst, p, kn, rn, rws)
    Wt = np.abs(tab.w[p, :ra, :rn].astype(np.float64))
    bb = np.abs(tab.bbar[p, :ra].astype(np.float64))
    absA = np.abs(A)
    rel = 2.0 ** -11 * (1 + 2.0 ** -10) if fp16 else 0.0
    sub = 2.0 ** -25 if fp16 else 0.0
    slack = np.sqrt(tab.dropped[p] + tab.eta[p])
    worst = 0.0
    for j, (s, t) in enumerate(zip(keep, slots)):
        c = sm.coef[p, t, :rn].astype(np.float64)
        lhs = U @ c + (mean if dc else 0.0)
        rhs = A @ B[:, s]
        elem = (rel * np.abs(U) + sub) @ np.abs(c) + (r + 3) * U32 * (absA @ (Wt @ np.abs(c) + (bb if dc else 0.0)))
        diff = np.linalg.norm(lhs - rhs)
        bound = np.linalg.norm(elem) + slack
        assert diff <= bound, (p, rws, j, diff, bound)
        worst = max(worst, diff / bound)
        # ... and from what a consumer reads, fp16 c_high and the dequantized c_low: additionally within the
        # quantizer's own step (fp16: 2^-11 |c'|, 2^-25 below the normal range; RTVQ: a code is at most one step of the
        # last stage, 1 / scale, from the residual it rounds -- the clamp at the range's ends included -- and the
        # dequantizing fp32 operations add 2^-22 of the stage values)
        cq = _dequantized(sm, p, t, kn, rn, orc)
        if np.isfinite(cq).all():
            step = np.zeros(rn)
            step[:kn] = np.maximum(2.0 ** -11 * np.abs(c[:kn]), 2.0 ** -25)
            if rn - kn >= 2:
                sc_ = sm.scale[p, t].astype(np.float64)
                step[kn:] = (1.0 + 2.0 ** -20) / sc_[-1] + 2.0 ** -21 * (np.abs(c[kn:]) + (2.0 ** dst.bits / sc_).sum())
                assert (np.abs(cq - c) <= step).all(), (p, t, float((np.abs(cq - c) / step).max()))
                lhs2 = U @ cq + (mean if dc else 0.0)
                assert np.linalg.norm(lhs2 - rhs) <= bound + np.linalg.norm(np.abs(U) @ step), (p, j)
    return worst


@pytest.mark.parametrize("n,fp16,sc,dc", SWEEP, ids=SWEEP_IDS)
def test_reconstruction_is_preserved(sq, orc, n, fp16, sc, dc):
    R = _run(n, fp16, sc, dc)
    for p, rws in enumerate(R["st"].rows):
        if rws:
            _check_property(R, p, list(range(n)), list(range(n)), fp16, dc, orc)


# ------------------------------------------------------------------------------------------ designed spectra
def _graded(n):
    """spectrum_cases.graded_sigmas' shape over half a decade: sigma_min / sigma_max = 10 ** -0.5."""
    return [10.0 ** (-0.5 * i / max(n - 1, 1)) for i in range(n)]


def _gap(n):
    """spectrum_cases.gap_sigmas' shape: n - 1 values falling gently to 10 ** -0.25, then 0.3."""
    return [10.0 ** (-0.25 * i / max(n - 2, 1)) for i in range(n - 1)] + [0.3]


@pytest.mark.parametrize("shape", ["graded", "gap"])
@pytest.mark.parametrize("n", [6, 8, 16, 20])
def test_designed_spectra(sq, orc, n, shape):
    """U orthonormal in fp64 then rounded to fp16, C = Sigma V^T with V orthogonal: an uncentred store whose task stack
    has the singular values designed, to the non-orthonormality of the rounded U.
      sigma'   Ur = U + E, |E_ij| <= 2^-11 |U_ij|, so ||E||_2 <= ||E||_F <= e := 2^-11 sqrt(n) and ||Ur^T Ur - I||_2 <= d :=
               2 e + e^2.  K = C^T (Ur^T Ur) C has eigenvalues theta_i sigma_i^2 with theta_i in [1 - d, 1 + d] (Ostrowski):
               the true sigma' is within d sigma_i / 2 (1 + d) of sigma_i.  The device's lambda' is within eta of the true
               lambda and, being kept, above 4 eta, so lambda >= 0.75 lambda', sigma >= 0.866 sigma' and
               |sqrt(lambda') - sqrt(lambda)| = |lambda' - lambda| / (sigma' + sigma) <= eta / (1.866 sigma'), sigma' the
               value the device reports (the issue's eta / (2 sigma_i) with the 25 % of the keep rule made explicit).
               Then the fp32 rounding.
      k'       a cumulative energy a / (a + b) whose terms each move by a relative eps <= 2.1 rel moves by at most
               2 eps cum (1 - cum) / (1 - eps); the threshold sits in the middle of a gap between two cumulative
               energies that is asserted to exceed that reach on both sides.
      U'^T U'  exactly, U' = Ur W has W^T (Ur^T Ur) W = I + Sigma^-1 V^T dK V Sigma^-1, |.|_ij <= eta / sqrt(lambda_i
               lambda_j).  Rounding U' to fp16 moves entry (i, j) by at most 2 * 2^-11 (1 + 2^-12) |u'_i| |u'_j| <= 1.1 *
               2^-10 with column norms <= 1.05; the fp32 chain ((n + 3) 2^-24 |Ur| |W|, |W| <= 1 / sigma_min) and the
               measuring Gram's own (256 + n + 3) 2^-24 are below 2^-15 each."""
    rows = 4097
    rng = np.random.default_rng(1000 * n + len(shape))
    sig = np.array(_graded(n) if shape == "graded" else _gap(n))
    assert sig.min() / sig.max() >= 0.1
    Q = np.linalg.qr(rng.standard_normal((rows, n)))[0]
    V = np.linalg.qr(rng.standard_normal((n, n)))[0]
    C = sig[:, None] * V.T
    # the coefficients the store holds are fp16 roundings of C: the spectrum designed is that of the rounded C
    C16 = C.astype(np.float16).astype(np.float64)
    s16 = np.linalg.svd(C16, compute_uv=False)
    cum = np.cumsum(s16 ** 2) / (s16 ** 2).sum()
    j = n - 1 if shape == "gap" else int(np.argmax(cum >= 0.9))
    thr = float(np.float32(0.5 * (cum[j - 1] + cum[j])))
    st = Store(n, fp16=True, center=False, rows=[rows], zero_at=None, made=[(Q, None, C)])
    dst = st.dst(center=False, thr=thr)
    sm, tab = st.plan.consolidate(dst, list(range(n)), rows_dev=st.rows_dev)
    assert int(sm.r[0]) == n
    e = 2.0 ** -11 * np.sqrt(n)
    d = 2 * e + e * e
    eta = float(tab.eta[0])
    got = sm.sigma[0, :n].astype(np.float64)
    bound = 0.5 * d * (1 + d) * s16 + eta / (1.866 * got) + 2.0 ** -23 * s16
    assert (np.abs(got - s16) <= bound).all(), (got, s16, bound)
    eps = 2.1 * float((bound / s16).max())
    for c in (cum[j - 1], cum[j]):
        assert abs(c - thr) > 2 * eps * c * (1 - c) / (1 - eps) + 2.0 ** -22, (cum, thr, eps)      # the fixture's gap
    assert int(sm.k[0]) == j + 1 == orc.select_rank(torch.from_numpy(s16.astype(np.float32)), thr, None)
    # orthonormality of the rounded U' through the store Gram of the DESTINATION (what basis_report reads)
    _, Bd = dst.store_gram(basis_gram=True)
    Bd = Bd[0].cpu().numpy()[:n, :n]
    lam = tab.lam[0, :n]
    lim = eta / np.sqrt(np.outer(lam, lam)) + 1.1 * 2.0 ** -10 + 2.0 ** -14
    defect = np.abs(Bd - np.eye(n))
    assert lim.max() < 0.05, float(lim.max())      # a wrong W (defect of order 1) cannot pass
    assert (defect <= lim).all(), float((defect / lim).max())


# ------------------------------------------------------------------------------------------ dropped tasks, degenerate stores
def _consolidated(st, dst, keep, **kw):
    _, M = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    st.plan.consolidate_eig(dst, keep, rows_dev=st.rows_dev, basis_gram=M, **kw)
    st.plan.rebase(dst, rows_dev=st.rows_dev)
    torch.cuda.synchronize()
    from oracle import svd_hybrid_oracle as orc
    ssm = _small_raw(st.plan)
    R = {"st": st, "dst": dst, "M": M.cpu().numpy(), "tab": _table(st.plan), "sm": _small_raw(dst), "ssm": ssm}
    R["src"] = [None if rws == 0 else _source(st.plan, ssm, p, rws, orc) for p, rws in enumerate(st.rows)]
    return R


def test_keep_three_of_eight(sq, orc):
    st = Store(8, fp16=True, center=True, rows=[257, 700], zero_at=None, shift=3)
    dst = st.dst(3, center=True)
    keep = [6, 1, 4]
    R = _consolidated(st, dst, keep)
    for p, rws in enumerate(st.rows):
        rn = int(R["tab"].r[p])
        assert 1 <= rn <= 2
        A, B = R["src"][p]
        kn = int(R["tab"].k[p])
        _, mean = _outputs(dst, p, kn, rn, rws)
        want = A @ B[:, keep].mean(axis=1)      # the kept tasks' mean
        r = st.kr[p][1]
        assert (np.abs(mean - want) <= (r + 4) * U32 * (np.abs(A) @ np.abs(B[:, keep]).mean(axis=1))).all()
        R["slots"] = [0, 1, 2]
        assert _check_eig(R, p, keep, True) == rn
        _check_property(R, p, keep, [0, 1, 2], True, True, orc)


def test_absent_destination_slots_are_zeros(sq, orc):
    st = Store(8, fp16=False, center=True, rows=[257], zero_at=None, shift=3)
    dst = st.dst(8, center=False)
    keep = [-1, 3, -1, 0, 7, -1, -1, 2]
    R = _consolidated(st, dst, keep)
    slots = [1, 3, 4, 7]
    kept = [3, 0, 7, 2]
    rn, kn = int(R["tab"].r[0]), int(R["tab"].k[0])
    assert 1 <= rn <= 4      # centred source to uncentred destination: the mean is folded into the data
    _check_tail(R["sm"], 0, 8, kn, rn, 4, STAGES, orc, slots=slots)
    _check_property(R, 0, kept, slots, False, False, orc)


def _made_store(C, rows=700, center=True, seed=0, fp16=True, mean_scale=1.0):
    rng = np.random.default_rng(seed)
    r, n = C.shape
    U = rng.standard_normal((rows, r)) / np.sqrt(rows)
    m = mean_scale * rng.standard_normal(rows) / np.sqrt(rows)
    return Store(n, fp16=fp16, center=center, rows=[rows], zero_at=None, made=[(U, m if center else None, C)])


def test_a_task_stored_twice(sq, orc):
    rng = np.random.default_rng(5)
    C = np.linalg.qr(rng.standard_normal((6, 6)))[0].astype(np.float16).astype(np.float64)      # six independent tasks
    st = _made_store(C)
    R0 = _consolidated(st, st.dst(6, center=True), list(range(6)))
    C[:, 4] = C[:, 1]
    st2 = _made_store(C)
    R1 = _consolidated(st2, st2.dst(6, center=True), list(range(6)))
    assert int(R0["tab"].r[0]) == 5 and int(R1["tab"].r[0]) == 4
    assert R1["tab"].dropped[0] <= 4 * R1["tab"].eta[0]      # about 0: what is dropped is below the noise floor
    _check_property(R1, 0, list(range(6)), list(range(6)), True, True, orc)


def test_all_tasks_equal(sq, orc):
    C = np.tile(np.array([[0.5], [-1.25], [2.0]]), (1, 5))
    st = _made_store(C)
    dst = st.dst(5, center=True)
    R = _consolidated(st, dst, list(range(5)))
    assert int(R["tab"].r[0]) == 0 and int(R["tab"].k[0]) == 0 and R["tab"].live[0] == 1
    assert not R["sm"].coef[0].any() and float(R["sm"].energy[0]) == 0.0
    A, B = R["src"][0]
    _, mean = _outputs(dst, 0, 0, 0, 700)
    assert (np.abs(mean - A @ B[:, 0]) <= 7 * U32 * (np.abs(A) @ np.abs(B[:, 0]))).all()      # the mean carries everything


@pytest.mark.parametrize("dc", [True, False], ids=["centred", "uncentred"])
def test_one_kept_task(sq, orc, dc):
    rng = np.random.default_rng(9)
    C = rng.standard_normal((4, 5)).astype(np.float16).astype(np.float64)
    st = _made_store(C)
    dst = st.dst(1, center=dc)
    R = _consolidated(st, dst, [2])
    assert int(R["tab"].r[0]) == (0 if dc else 1)
    R["slots"] = [0]
    _check_eig(R, 0, [2], dc)
    _check_property(R, 0, [2], [0], True, dc, orc)


def test_zero_store(sq, orc):
    st = Store(3, fp16=True, center=True, rows=[257], zero_at=None,
               made=[(np.zeros((257, 2)), np.zeros(257), np.zeros((2, 3)))])
    dst = st.dst(3, center=True)
    _sentinel(dst)
    R = _consolidated(st, dst, [0, 1, 2])
    assert int(R["tab"].r[0]) == 0 and R["tab"].dropped[0] == 0.0 and R["tab"].eta[0] == 0.0
    _, mean = _outputs(dst, 0, 0, 0, 257)
    assert not mean.any()
    assert not R["sm"].sigma[0].any() and int(R["sm"].rows[0]) == 257


def test_no_kept_task_and_min_sigma(sq, orc):
    st = Store(8, fp16=True, center=True, rows=[257, 700], zero_at=None, shift=3)
    dst = st.dst(8, center=True)
    _sentinel(dst)
    keep = np.array([[-1] * 8, list(range(8))])
    R = _consolidated(st, dst, keep, min_sigma=0.5)
    assert R["tab"].live[0] == 0 and int(R["sm"].rows[0]) == 0 and not R["sm"].coef[0].any()
    o, nb = dst.slab_off[0], dst.slab_off[1]
    assert (dst.basis[o:nb].cpu().numpy() == SENT).all()      # no row of the entry without a kept task is written
    assert (dst.mean[:257].view(torch.uint8).cpu().numpy() == SENT).all()
    lam = R["tab"].lam[1, :8]
    rn = int(R["tab"].r[1])
    assert rn == int((lam > max(4 * R["tab"].eta[1], 0.25 * lam[0])).sum()) and rn >= 1
    _check_eig(R, 1, list(range(8)), True, min_sigma=0.5)


# ------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("where", ["U", "mean", "scale"])
def test_non_finite_store_is_flagged(sq, orc, where):
    from svdq_amd.pipeline import NonFiniteInput
    st = Store(8, fp16=True, center=True, rows=[257, 700, 13], zero_at=None, shift=3)      # entry 1: k = 0, r = 8
    if where == "U":
        st.us[1][300, 2] = float("nan")
    elif where == "mean":
        st.means[1][699] = float("nan")
    else:
        st.entries[1]["scale"][5, 1] = np.float32("nan")
    st.upload()
    dst = st.dst(8, center=True)
    _sentinel(dst)
    with pytest.raises(NonFiniteInput) as ei:
        st.plan.consolidate(dst, list(range(8)), rows_dev=st.rows_dev)
    assert ei.value.indices == [1]
    sm, tab = _small_raw(dst), _table(st.plan)
    assert np.isnan(sm.energy[1]) and np.isnan(sm.sigma[1]).all() and int(sm.rows[1]) == 700
    assert 0 <= int(sm.k[1]) <= int(sm.r[1]) <= 8 and not tab.w[1].any() and tab.live[1] == 0
    # the other entries are unaffected: the same bytes as a clean store gives them
    clean = Store(8, fp16=True, center=True, rows=[257, 700, 13], zero_at=None, shift=3)
    cd = clean.dst(8, center=True)
    csm, ctab = clean.plan.consolidate(cd, list(range(8)), rows_dev=clean.rows_dev)
    for p in (0, 2):
        assert np.array_equal(sm.coef[p], csm.coef[p]) and np.array_equal(sm.sigma[p], csm.sigma[p])
        assert np.array_equal(tab.w[p], ctab.w[p]) and int(sm.k[p]) == int(csm.k[p])
        rn, kn = int(ctab.r[p]), int(ctab.k[p])
        for a, b in zip(dst.basis_tensors(p, kn, rn, st.rows[p]), cd.basis_tensors(p, kn, rn, st.rows[p])):
            assert torch.equal(a, b)


def test_refusals_come_before_any_launch(sq):
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import CompressPlan, _stream_ptr
    lib = nat.lib()
    st = Store(8, fp16=True, center=True, rows=[257, 700], zero_at=None, shift=3)
    dst = st.dst(8, center=True)
    _sentinel(dst)
    dst.small.fill_(SENT)
    _, M = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    lay = st.plan.consolidate_layout()
    tab = torch.full((int(lay.total_bytes),), SENT, dtype=torch.uint8, device=st.dev)
    keep = np.ascontiguousarray(np.tile(np.arange(8, dtype=np.int32), (2, 1)))
    kd = torch.from_numpy(keep).to(st.dev)
    V = ctypes.c_void_p

    def eig(src=st.plan._h, d=dst._h, kh=keep.ctypes.data, kdev=kd.data_ptr(), rows=st.rows_dev.data_ptr(),
            ss=st.plan.small.data_ptr(), m=M.data_ptr(), ms=0.0, ds=dst.small.data_ptr(), tb=tab.data_ptr()):
        return lib.svdq_plan_consolidate_eig(src, d, V(kh), V(kdev), V(rows), V(ss), V(m), ms, V(ds), V(tb), _stream_ptr())

    def reb(src=st.plan._h, d=dst._h, rows=st.rows_dev.data_ptr(), ss=st.plan.small.data_ptr(),
            sb=st.plan.basis.data_ptr(), smn=st.plan.mean.data_ptr(), tb=tab.data_ptr(), db=dst.basis.data_ptr(),
            dm=dst.mean.data_ptr()):
        return lib.svdq_plan_rebase(src, d, V(rows), V(ss), V(sb), V(smn), V(tb), V(db), V(dm), _stream_ptr())

    E = nat.SVDQ_EINVAL
    for name in ("src", "d", "kh", "kdev", "ss", "m", "ds", "tb"):
        assert eig(**{name: None}) == E, name
    for name in ("src", "d", "ss", "sb", "smn", "tb", "db", "dm"):
        assert reb(**{name: None}) == E, name
    assert eig(kdev=kd.data_ptr() + 4) == E and eig(rows=st.rows_dev.data_ptr() + 4) == E      # tables off 8
    assert eig(m=M.data_ptr() + 4) == E and reb(rows=st.rows_dev.data_ptr() + 4) == E
    for name in ("ss", "ds", "tb"):                                                            # buffers off 16
        assert eig(**{name: tab.data_ptr() + 8}) == E, name
    for name in ("ss", "sb", "smn", "tb", "db", "dm"):
        assert reb(**{name: tab.data_ptr() + 8}) == E, name
    other_rows = CompressPlan([257, 701], 8, fp16=True, device=st.dev, unit_rows=UNIT_ROWS, workspace=False)
    other_type = CompressPlan([257, 700], 8, fp16=False, device=st.dev, unit_rows=UNIT_ROWS, workspace=False)
    other_p = CompressPlan([257], 8, fp16=True, device=st.dev, unit_rows=UNIT_ROWS, workspace=False)
    for o in (other_rows, other_type, other_p):
        assert eig(d=o._h) == E and reb(d=o._h) == E
    with pytest.raises(ValueError):      # N' > SVDQ_MAX_TASKS: no such plan can be made
        CompressPlan([257, 700], 33, fp16=True, device=st.dev, workspace=False)
    for bad in (-2, 8):
        k2 = keep.copy()
        k2[1, 3] = bad
        assert eig(kh=k2.ctypes.data) == E, bad
    for ms in (-0.5, float("nan"), float("inf")):
        assert eig(ms=ms) == E, ms
    lo = nat.SvdqConsolidateLayout()
    assert lib.svdq_plan_consolidate_layout(None, ctypes.byref(lo)) == E
    assert lib.svdq_plan_consolidate_layout(st.plan._h, None) == E
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its sentinel
    for t in (tab, dst.small, dst.basis, dst.mean.view(torch.uint8)):
        assert bool((t == SENT).all())
    assert eig() == nat.SVDQ_OK and reb() == nat.SVDQ_OK
    torch.cuda.synchronize()
    # the host layer's own refusals
    with pytest.raises(ValueError):
        st.plan.consolidate_eig(dst, [0, 1, 2], rows_dev=st.rows_dev)      # not N' entries
    with pytest.raises(ValueError):
        st.plan.consolidate_eig(dst, [0, 1, 2, 3, 4, 5, 6, 8], rows_dev=st.rows_dev)
