"""
GPU tests of svdq_plan_store_gram (include/svdq.h; CompressPlan.store_gram): the N x N Gram of the task vectors a
plan's stored artifacts reconstruct, from one pass over the basis and the mean.

Truth: numpy fp64 on the very artifacts the kernel reads -- the plan's basis and mean buffers and its small buffer,
copied back -- Delta = U C + mean with C from the fp16 c_high and the c_low dequantized by the C model of the
quantizer (the device lines are bit-exact to it), G = Delta^T Delta.

Bound, per entry: |G - G64|[t][s] <= (256 + r + 3) 2^-24 (|C'|^T (|A|^T |A|) |C'|)[t][s] with A = [U | mean] and
C' = [C ; 1]: A^T A is a sum of fp32 partial sums over at most 256 rows each (gamma_256 relative to |A|^T |A|, in any
order), added in fp64; the coefficients are exact (the dequantizer is bit-exact), and r + 3 covers the fp64 steps with
room to spare.  Derived, not fitted.

Every adopted plan is filled by svdq_plan_import from tensors made here: U is random and NOT orthonormal (entries
around 1 / sqrt(D), columns correlated through a shared component), so a kernel that takes U^T U = I fails; codes,
scales and zero points are random and finite.  Spikes of 1e3 x the typical magnitude sit in U and the mean at the first
and last rows of blocks, units and the parameter, so a dropped or doubled row exceeds the bound at any D.
"""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SENT = 0xA5
ROWS = [1, 3, 13, 63, 64, 255, 256, 257, 4095, 4096, 4097, 8193, 70001, 127, 128, 129, 513]      # + RB = 128's edges, 2 RB + 1
TASKS = [1, 3, 8, 16, 17, 32]
KINDS = ["r1k0", "r1k1", "rNk0", "rNk1", "rNkr"]
SPIKES = [0, 63, 64, 255, 256, 4095, 4096]
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


def _kr(rows, n, kind):
    r = 1 if kind.startswith("r1") else n
    r = min(r, rows, n)
    k = {"k0": 0, "k1": 1, "kr": r}[kind[2:]]
    return min(k, r), r


class Store:
    """A ragged adopted plan: one parameter per entry of ``rows`` (None = a parameter whose rows_dev is 0)."""

    def __init__(self, n, *, fp16, center, kind, rows=ROWS, zero_at=3, bits=4, seed=0):
        from svdq_amd.pipeline import CompressPlan, pack_small
        dev = torch.device("cuda", 0)
        rows = list(rows)
        if zero_at is not None:
            rows.insert(zero_at, None)
        g = torch.Generator().manual_seed(7919 * n + 31 * seed + KINDS.index(kind))
        self.n, self.fp16, self.center, self.dev = n, fp16, center, dev
        self.rows = [r if r is not None else 0 for r in rows]
        plan_rows = [r if r is not None else 300 for r in rows]
        self.plan = CompressPlan(plan_rows, n, center=center, fp16=fp16, low_bits=bits, rtvq_stages=STAGES, device=dev,
                                 unit_rows=UNIT_ROWS, workspace=False)
        udt = torch.float16 if fp16 else torch.float32
        self.kr, us, means, entries = [], [], [], []
        for rws in rows:
            if rws is None:
                self.kr.append((0, 0))
                us.append(None)
                means.append(None)
                entries.append(None)
                continue
            k, r = _kr(rws, n, kind)
            typ = 1.0 / np.sqrt(rws)
            u = (torch.randn(rws, r, generator=g) + 0.5 * torch.randn(rws, 1, generator=g)) * typ
            m = torch.randn(rws, generator=g) * typ
            for s in SPIKES + [rws - 1]:
                if s < rws:
                    u[s] = 1.0e3 * typ * (1.0 + 0.25 * torch.rand(r, generator=g))
                    m[s] = -1.0e3 * typ
            self.kr.append((k, r))
            us.append(u.to(udt))
            means.append(m)
            q = 1 << bits
            entries.append({
                "rows": rws, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
                "c_high": torch.randn(n, k, generator=g).numpy().astype(np.float16),
                "codes": torch.randint(0, q, (n, STAGES, r - k), generator=g).numpy().astype(np.uint8),
                "scale": (2.0 + 30.0 * torch.rand(n, STAGES, generator=g)).numpy().astype(np.float32),
                "zero_point": torch.randint(0, q, (n, STAGES), generator=g).numpy().astype(np.float32),
                "residual_norm": np.zeros((n, STAGES), np.float32)})
        host = pack_small(self.plan.layout, len(rows), n, STAGES, entries)
        uh = [None if u is None else u[:, :k].contiguous().to(dev) for u, (k, r) in zip(us, self.kr)]
        ul = [None if u is None else u[:, k:].contiguous().to(dev) for u, (k, r) in zip(us, self.kr)]
        mn = [None if m is None else m.to(dev) for m in means] if center else None
        self.plan.import_artifacts(uh, ul, mn, host)
        self.rows_dev = torch.tensor(self.rows, dtype=torch.int64).to(dev)


def _artifacts(plan, sm, p, rows, orc):
    """(A [rows, r (+ 1)], C' [r (+ 1), N]) in fp64 from the plan's own buffers: what the kernel reads."""
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


def _check_param(G, A, C, r, where):
    assert np.isfinite(A).all() and np.isfinite(C).all(), where
    delta = A @ C
    G64 = delta.T @ delta
    bound = (256 + r + 3) * U32 * (np.abs(C).T @ (np.abs(A).T @ np.abs(A)) @ np.abs(C))
    err = np.abs(G - G64)
    assert (err <= bound).all(), (where, float((err / np.maximum(bound, 1e-300)).max()))
    assert np.array_equal(G, G.T), where


def _check_plan(plan, rows, G, orc, B=None, where=""):
    sm = plan.fetch_small()
    G = G.cpu().numpy()
    B = None if B is None else B.cpu().numpy()
    for p, rws in enumerate(rows):
        if rws == 0:
            assert not G[p].any(), (where, p)
            assert B is None or not B[p].any(), (where, p)
            continue
        r = int(sm.r[p])
        A, C = _artifacts(plan, sm, p, rws, orc)
        _check_param(G[p], A, C, r, (where, p, rws))
        if B is not None:
            ra = A.shape[1]
            B64 = A.T @ A
            bb = (256 + r + 3) * U32 * (np.abs(A).T @ np.abs(A))
            assert (np.abs(B[p][:ra, :ra] - B64) <= bb).all(), (where, p, rws)
            assert np.array_equal(B[p], B[p].T), (where, p)
            rest = B[p].copy()
            rest[:ra, :ra] = 0.0
            assert not rest.any(), (where, p)


# ------------------------------------------------------------------------------------------ adopted plans
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("n", TASKS)
def test_adopted_plan_against_fp64(sq, orc, n, fp16, center, kind):
    st = Store(n, fp16=fp16, center=center, kind=kind)
    G, B = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    G2 = st.plan.store_gram(rows_dev=st.rows_dev)
    assert torch.equal(G, G2)                      # the same bits in every run
    _check_plan(st.plan, st.rows, G, orc, B=B, where=(n, fp16, center, kind))


def test_rows_default_to_the_small_buffer(sq, orc):
    """rows_dev = None: the rows field of the small buffer, read on the device (a rows = 0 entry there is skipped)."""
    st = Store(8, fp16=True, center=True, kind="rNk1", rows=[257, 4097, 13])
    G = st.plan.store_gram()
    assert torch.equal(G, st.plan.store_gram(rows_dev=st.rows_dev))
    _check_plan(st.plan, st.rows, G, orc)


# ------------------------------------------------------------------------------------------ a fused run's plan
@pytest.mark.parametrize("n", [8, 20])
def test_fused_plan(sq, orc, n):
    """compress_batch's own plan: the same check, and G is within rtol 2e-6 / atol 2e-6 max|G| of the fp64 Gram of the
    ORIGINAL deltas only if the reference chain's own reconstruction is -- a condition computed with the CPU model and
    asserted for this seed: it is False (fp16 c_high and a 4-bit c_low move the Gram by several 1e-4)."""
    D, seed, thr = 4097, 3, 0.9
    deltas = orc.synthetic_deltas(D, n, seed)
    ref = orc.compress_parameter(deltas, thr, None, True, True, 4, 2)
    X = torch.stack(deltas, 1).double().numpy()
    R = torch.stack(ref["recon"], 1).double().numpy()
    G0, G1 = X.T @ X, R.T @ R

    def close(g):
        return bool(np.allclose(g, G0, rtol=2e-6, atol=2e-6 * np.abs(G0).max()))

    cond = close(G1)
    assert cond is False
    dev = torch.device("cuda", 0)
    plan, sm = sq.compress_batch([[d.to(dev) for d in deltas]], energy_threshold=thr, max_rank=None, center=True,
                                 fp16=True, low_bits=4, rtvq_stages=2, device=dev)
    k, r = int(sm.k[0]), int(sm.r[0])
    assert r - k >= 3, (k, r)
    G = plan.store_gram()
    assert torch.equal(G, plan.store_gram())
    A, C = _artifacts(plan, sm, 0, D, orc)
    assert np.isfinite(A).all() and np.isfinite(C).all()
    _check_param(G[0].cpu().numpy(), A, C, r, ("fused", n))
    assert (not close(G[0].cpu().numpy())) or cond


# ------------------------------------------------------------------------------------------ an extended basis
def test_extended_basis_is_orthonormal_to_fp16(sq, orc):
    """A plan grown by svdq_plan_extend_basis (N = 8, one new task): basis_gram reports max |U^T U - I| < 2^-9 -- the
    stored columns are fp16 roundings of orthonormal ones (2^-11 relative per element), the new one is orthogonalised
    against them in fp32 and rounded the same way."""
    from svdq_amd.pipeline import CompressPlan, pack_small
    dev = torch.device("cuda", 0)
    n, rows, r = 8, 4097, 7
    g = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(rows, r + 1, generator=g, dtype=torch.float64))
    u = q[:, :r].contiguous().half()
    mean = torch.randn(rows, generator=g) * 0.01

    def entry(k, rr):
        return {"rows": rows, "k": k, "r": rr, "energy": 0.5, "sigma": np.ones(rr, np.float32),
                "c_high": np.zeros((n, k), np.float16), "codes": np.zeros((n, STAGES, rr - k), np.uint8),
                "scale": np.ones((n, STAGES), np.float32), "zero_point": np.zeros((n, STAGES), np.float32),
                "residual_norm": np.zeros((n, STAGES), np.float32)}

    plan = CompressPlan([rows], n, center=True, fp16=True, device=dev, unit_rows=UNIT_ROWS, workspace=False)
    empty = torch.empty((rows, 0), dtype=torch.float16, device=dev)
    plan.import_artifacts([u.to(dev)], [empty], [mean.to(dev)], pack_small(plan.layout, 1, n, STAGES, [entry(r, r)]))
    x = (mean.double() + u.double() @ torch.randn(r, generator=g, dtype=torch.float64) + 0.7 * q[:, r]).float().to(dev)
    table = torch.tensor([x.data_ptr()] + [0] * (n - 1), dtype=torch.int64).to(dev)
    plan.project_tasks(table)
    ext = plan.residual_gram(table, 1)
    assert int(ext.m[0]) == 1
    out = torch.empty((rows, r + 1), dtype=torch.float16, device=dev)
    plan.extend_basis(table, 1, [out])
    grown = CompressPlan([rows], n, center=True, fp16=True, device=dev, unit_rows=UNIT_ROWS, workspace=False)
    grown.import_artifacts([out], [empty], [mean.to(dev)], pack_small(grown.layout, 1, n, STAGES, [entry(r + 1, r + 1)]))
    G, B = grown.store_gram(basis_gram=True)
    B = B[0].cpu().numpy()
    dev_from_I = np.abs(B[:r + 1, :r + 1] - np.eye(r + 1)).max()
    assert dev_from_I < 2.0 ** -9, dev_from_I
    _check_plan(grown, [rows], G, orc, B=torch.from_numpy(B)[None])


# ------------------------------------------------------------------------------------------ the entry point
def _raw_call(st, lib, G, B, *, plan=True, small=True, basis=True, mean=True, work=True, rows=None, off=0):
    from svdq_amd.pipeline import _ptr, _stream_ptr
    pl = st.plan
    need = int(lib.svdq_plan_store_gram_work_bytes(pl._h))
    if getattr(st, "_work", None) is None:
        st._work = torch.empty(need + 64, dtype=torch.uint8, device=st.dev)
    p = lambda t, on=True: ctypes.c_void_p((t.data_ptr() + off) if (on and t is not None) else 0)
    return lib.svdq_plan_store_gram(pl._h if plan else None, _ptr(st.rows_dev if rows is None else rows),
                                    p(pl.small, small), p(pl.basis, basis), p(pl.mean, mean), p(st._work, work),
                                    _ptr(G), _ptr(B), _stream_ptr())


def test_refusals_come_before_any_launch(sq):
    from svdq_amd import _native as nat
    lib = nat.lib()
    st = Store(8, fp16=True, center=True, kind="rNk1", rows=[257, 4097], zero_at=None)
    P, n = len(st.rows), st.n
    G = torch.full((P, n, n), -7.0, dtype=torch.float64, device=st.dev)
    B = torch.full((P, 33, 33), -7.0, dtype=torch.float64, device=st.dev)
    for what in ("plan", "small", "basis", "mean", "work"):
        assert _raw_call(st, lib, G, B, **{what: False}) == nat.SVDQ_EINVAL, what
    assert _raw_call(st, lib, None, B) == nat.SVDQ_EINVAL
    assert _raw_call(st, lib, G, B, off=4) == nat.SVDQ_EINVAL      # small / basis / mean off 16, work off 8
    odd = torch.zeros(P + 1, dtype=torch.int64, device=st.dev)
    assert lib.svdq_plan_store_gram(st.plan._h, ctypes.c_void_p(odd.data_ptr() + 4), ctypes.c_void_p(st.plan.small.data_ptr()),
                                    ctypes.c_void_p(st.plan.basis.data_ptr()), ctypes.c_void_p(st.plan.mean.data_ptr()),
                                    ctypes.c_void_p(st._work.data_ptr()), ctypes.c_void_p(G.data_ptr()), None,
                                    None) == nat.SVDQ_EINVAL
    assert lib.svdq_plan_store_gram_work_bytes(None) == 0
    torch.cuda.synchronize()
    assert bool((G == -7.0).all()) and bool((B == -7.0).all())      # nothing was launched
    assert _raw_call(st, lib, G, B) == nat.SVDQ_OK
    # an uncentred plan ignores the mean
    nc = Store(8, fp16=True, center=False, kind="rNk1", rows=[257], zero_at=None)
    Gn = torch.empty((1, n, n), dtype=torch.float64, device=st.dev)
    assert _raw_call(nc, lib, Gn, None, mean=False) == nat.SVDQ_OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,fp16", [(8, True), (20, False)])
def test_nothing_is_written_outside_the_outputs(sq, n, fp16):
    """The outputs carved out of one sentinel-filled buffer: the gaps before, between and behind them keep the
    sentinel, and so do the plan's own buffers their bytes."""
    from svdq_amd import _native as nat
    lib = nat.lib()
    st = Store(n, fp16=fp16, center=True, kind="rNk1", rows=[257, 4097, 13])
    P = len(st.rows)
    gb, bb, gap = P * n * n * 8, P * 33 * 33 * 8, 4096
    buf = torch.full((3 * gap + gb + bb,), SENT, dtype=torch.uint8, device=st.dev)
    G = buf[gap:gap + gb].view(torch.float64).view(P, n, n)
    B = buf[2 * gap + gb:2 * gap + gb + bb].view(torch.float64).view(P, 33, 33)
    before = [st.plan.small.clone(), st.plan.basis.clone(), st.plan.mean.clone()]
    assert _raw_call(st, lib, G, B) == nat.SVDQ_OK
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    for a, b in ((0, gap), (gap + gb, 2 * gap + gb), (2 * gap + gb + bb, host.size)):
        assert (host[a:b] == SENT).all(), (a, b)
    assert torch.equal(G, st.plan.store_gram(rows_dev=st.rows_dev))
    for was, now in zip(before, [st.plan.small, st.plan.basis, st.plan.mean]):
        assert torch.equal(was, now)


def test_capture_and_two_replays(sq):
    st = Store(8, fp16=True, center=True, kind="rNk1", rows=[257, 4097, 13])
    want, want_b = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)      # also sizes the cached work buffer
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            G, B = st.plan.store_gram(rows_dev=st.rows_dev, basis_gram=True)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        G.fill_(-1.0)
        B.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(G, want) and torch.equal(B, want_b)
