"""
GPU tests of svdq_plan_project (include/svdq.h; CompressPlan.project_tasks): new task tensors projected onto the basis a
plan already holds, and the coefficient epilogue behind it.

Every plan here is filled with svdq_plan_import from tensors the test made itself, so k, r and the basis are free:
k = 0, k = r, r = N and r < N sit side by side in one plan, next to a parameter with rows = 0.  Shapes are the smallest
at which a block, a unit or a tail can go wrong: 1 row, around the 256-row block, 1027 rows in five 256-row units.

The truth bound (check 1) is derived, not measured: a coefficient is a sum of fp32 partial sums over at most 256 rows
each, added in fp64.  A 256-term fp32 sum of rounded products, in any order, is within gamma_256 <= 256 u / (1 - 256 u)
of the exact sum relative to sum |U||xc| (u = 2^-24); the fp64 part and the last rounding to fp32 add u |c|.  258 u
covers gamma_256 with the fp64 terms to spare.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 0xA5
TASK_COUNTS = [1, 3, 8, 9, 16, 17, 20, 32]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle as o
    o.build_c_oracle()
    return o


def _kr(rows, n, which):
    """(k, r) of the four kinds the issue names, held to r <= min(rows, N)."""
    rmax = min(rows, n)
    if which == "k0":
        return 0, rmax
    if which == "k=r":
        return rmax, rmax
    if which == "r=N":
        return min(1, rmax), rmax
    r = max(1, rmax - 1)      # r < N where there is room
    return r // 2, r


# (rows of the basis, kind) of the parameters of the standard plan; rows None = a parameter whose rows are 0
# the block edges of both block sizes (256 rows up to 16 slots, 128 above): 1, RB - 1, RB, RB + 1, 2 RB + 1
STANDARD = [(1, "k=r"), (255, "k0"), (256, "k=r"), (257, "r<N"), (None, "k0"), (1027, "r=N"),
            (127, "r<N"), (128, "k=r"), (129, "k0"), (513, "r=N")]


class Plan:
    """A plan filled by svdq_plan_import from random tensors: U [rows, r] in the basis dtype, mean [rows]."""

    def __init__(self, sq, n, *, fp16, center, params=STANDARD, bits=4, stages=2, unit_rows=256,
                 input_dtype=torch.float32, seed=0, sentinel=True):
        from svdq_amd.pipeline import CompressPlan, pack_small
        dev = torch.device("cuda", 0)
        g = torch.Generator().manual_seed(1000 * n + seed)
        self.n, self.fp16, self.center = n, fp16, center
        self.rows = [r if r is not None else 0 for r, _ in params]
        plan_rows = [r if r is not None else 300 for r, _ in params]
        bits_list = list(bits) if isinstance(bits, (list, tuple)) else [bits] * len(params)
        self.bits = bits_list
        self.plan = CompressPlan(plan_rows, n, center=center, fp16=fp16, low_bits=bits_list, rtvq_stages=stages,
                                 device=dev, unit_rows=unit_rows, input_dtype=input_dtype, workspace=False)
        udt = torch.float16 if fp16 else torch.float32
        self.kr, self.U, self.mean, entries = [], [], [], []
        for rows, kind in params:
            if rows is None:
                self.kr.append((0, 0))
                self.U.append(None)
                self.mean.append(None)
                entries.append(None)
                continue
            k, r = _kr(rows, n, kind)
            u = (torch.randn(rows, r, generator=g) / np.sqrt(rows)).to(udt)
            m = torch.randn(rows, generator=g) * 0.01
            self.kr.append((k, r))
            self.U.append(u)
            self.mean.append(m if center else None)
            entries.append({"rows": rows, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
                            "c_high": np.zeros((n, k), np.float16), "codes": np.zeros((n, stages, r - k), np.uint8),
                            "scale": np.zeros((n, stages), np.float32), "zero_point": np.zeros((n, stages), np.float32),
                            "residual_norm": np.zeros((n, stages), np.float32)})
        L = self.plan.layout
        host = pack_small(L, len(params), n, stages, entries)
        if sentinel:      # everything the projection may write starts as a sentinel
            host[L.chigh_off:L.status_off] = SENTINEL
        uh = [None if u is None else u[:, :k].contiguous().to(dev) for u, (k, r) in zip(self.U, self.kr)]
        ul = [None if u is None else u[:, k:].contiguous().to(dev) for u, (k, r) in zip(self.U, self.kr)]
        mn = [None if m is None else m.to(dev) for m in self.mean] if center else None
        self.plan.import_artifacts(uh, ul, mn, host)
        self.rows_dev = torch.tensor(self.rows, dtype=torch.int64).to(dev)
        self.dev = dev
        self._keep = []

    def table(self, tensors):
        """tensors[p][t] (None = absent slot) -> the int64 device table (raw addresses: the owners are kept alive)."""
        self._keep.append(tensors)
        return torch.tensor([0 if t is None else t.data_ptr() for ts in tensors for t in ts], dtype=torch.int64).to(self.dev)

    def ptrs(self, tensors):
        self._keep.append(tensors)      # every table's tensors stay alive as long as the plan
        return torch.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch.int64).to(self.dev)

    def small_bytes(self):
        return self.plan.small.cpu().numpy().copy()


def _inputs(pl, seed=1, absent=()):
    """x[p][t]: fp32 CPU tensors of rows[p] elements (one element for a rows = 0 parameter, never read)."""
    g = torch.Generator().manual_seed(seed)
    return [[None if (p, t) in absent else torch.randn(max(rows, 1), generator=g) for t in range(pl.n)]
            for p, rows in enumerate(pl.rows)]


def _cuda(xs):
    return [[None if x is None else x.cuda() for x in row] for row in xs]


def _truth(pl, p, x):
    """(c_ref [r] fp64, the bound's sum |U||xc| [r]) for one fp32 vector, from the tensors the kernel reads."""
    xc = x.float()
    if pl.mean[p] is not None:
        xc = xc - pl.mean[p]            # one fp32 subtraction
    u = pl.U[p].double()
    return u.T @ xc.double(), u.abs().T @ xc.double().abs()


def _assert_truth(pl, sm, xs):
    for p, rows in enumerate(pl.rows):
        if rows == 0:
            continue
        k, r = pl.kr[p]
        for t in range(pl.n):
            if xs[p][t] is None:
                continue
            ref, mag = _truth(pl, p, xs[p][t])
            c = torch.from_numpy(sm.coef[p, t, :r].copy()).double()
            err = (c - ref).abs()
            bound = 258 * U * mag + U * ref.abs()
            assert bool((err <= bound).all()), (p, t, float((err / bound.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("n", TASK_COUNTS)
def test_truth(sq, n, fp16, center):
    pl = Plan(sq, n, fp16=fp16, center=center)
    xs = _inputs(pl)
    sm = pl.plan.project_tasks(pl.table(_cuda(xs)), rows_dev=pl.rows_dev)
    assert sm.rows.tolist() == pl.rows
    _assert_truth(pl, sm, xs)


# ------------------------------------------------------------------------------------------ 2. spikes
@pytest.mark.parametrize("n", [16, 20])
def test_spikes(sq, n):
    """One large element on a zero background at the first and last row of a block, a unit and the parameter: the
    coefficient is that single product, so a dropped or doubled row shows at any size."""
    rows = 1027
    pl = Plan(sq, n, fp16=False, center=False, params=[(rows, "r=N")], unit_rows=512)
    spikes = [0, 127, 128, 255, 256, 511, 512, 767, 768, 1023, 1024, 1026]
    assert len(spikes) <= n
    xs = [[torch.zeros(rows) for _ in range(n)]]
    for t, s in enumerate(spikes):
        xs[0][t][s] = 3.0e4 + t
    sm = pl.plan.project_tasks(pl.table(_cuda(xs)))
    k, r = pl.kr[0]
    for t in range(n):
        c = torch.from_numpy(sm.coef[0, t, :r].copy()).double()
        if t < len(spikes):
            s = spikes[t]
            assert bool(pl.U[0][s].abs().min() > 0)
            ref = pl.U[0][s].double() * float(xs[0][t][s])
            assert bool(((c - ref).abs() <= U * ref.abs()).all()), (t, s)
        else:
            assert not c.any()


# ------------------------------------------------------------------------------------------ 3. inputs
def _coef_fields(pl):
    L = pl.plan.layout
    return pl.small_bytes()[L.chigh_off:L.status_off]


@pytest.mark.parametrize("n", [8, 20])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_from_base_and_half_inputs_are_the_plain_call_bit_for_bit(sq, n, dtype):
    params = [(255, "k0"), (257, "r<N"), (1027, "r=N")]
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(r, generator=g).to(dtype) for r, _ in params]
    ft = [[(base[p].float() + 0.02 * torch.randn(r, generator=g)).to(dtype) for _ in range(n)]
          for p, (r, _) in enumerate(params)]
    # the plain fp32 call on tensors holding (float)finetuned - (float)base
    ref = Plan(sq, n, fp16=True, center=True, params=params)
    delta = [[f.float() - base[p].float() for f in row] for p, row in enumerate(ft)]
    ref.plan.project_tasks(ref.table(_cuda(delta)))
    want = _coef_fields(ref)
    # straight from checkpoints in their own dtype
    pl = Plan(sq, n, fp16=True, center=True, params=params, input_dtype=dtype)
    pl.plan.project_tasks(pl.table(_cuda(ft)), base_table=pl.ptrs([b.cuda() for b in base]))
    assert np.array_equal(_coef_fields(pl), want)
    # half deltas read as they are against their fp32 copies
    if dtype is not torch.float32:
        half = [[d.to(dtype) for d in row] for row in delta]
        a = Plan(sq, n, fp16=True, center=True, params=params, input_dtype=dtype)
        a.plan.project_tasks(a.table(_cuda(half)))
        b = Plan(sq, n, fp16=True, center=True, params=params)
        b.plan.project_tasks(b.table(_cuda([[h.float() for h in row] for row in half])))
        assert np.array_equal(_coef_fields(a), _coef_fields(b))


@pytest.mark.parametrize("n", [8, 20])
@pytest.mark.parametrize("with_base", [False, True], ids=["gather", "gather+base"])
def test_index_lists_are_the_plain_call_on_gathered_rows(sq, n, with_base):
    numel = 1500
    g = torch.Generator().manual_seed(9)
    mask = torch.rand(numel, generator=g) < 0.6
    mask[100:180] = False          # gaps
    mask[-7:] = torch.tensor([True, False, True, True, False, False, True])      # a ragged tail
    idx = [torch.nonzero(mask).flatten().int(), torch.nonzero(~mask).flatten().int()]      # the list and its inverse
    params = [(int(i.numel()), kind) for i, kind in zip(idx, ("r=N", "r<N"))]
    base = torch.randn(numel, generator=g)
    full = [base + 0.02 * torch.randn(numel, generator=g) for _ in range(n)]
    src = full if with_base else [f - base for f in full]
    ref = Plan(sq, n, fp16=False, center=True, params=params)
    gathered = [[(f[i.long()] - base[i.long()]) for f in full] for i in idx]
    ref.plan.project_tasks(ref.table(_cuda(gathered)))
    pl = Plan(sq, n, fp16=False, center=True, params=params)
    dev_src = [s.cuda() for s in src]
    pl.plan.project_tasks(pl.table([dev_src, dev_src]), index_table=pl.ptrs([i.cuda() for i in idx]),
                          base_table=pl.ptrs([base.cuda()] * 2) if with_base else None, rows_dev=pl.rows_dev)
    assert np.array_equal(_coef_fields(pl), _coef_fields(ref))


# ------------------------------------------------------------------------------------------ 4. epilogue
def _assert_epilogue(sq, orc, pl, sm, xs, stages):
    def same_bits(a, b):
        """Bit for bit; a NaN (a degenerate stage: range 0, scale inf) equals a NaN whatever its payload."""
        a, b = (np.ascontiguousarray(np.asarray(x, dtype=np.float32)) for x in (a, b))
        return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())

    for p, rows in enumerate(pl.rows):
        if rows == 0:
            continue
        k, r = pl.kr[p]
        nl = r - k
        quant = sq.RTVQQuantizer(pl.bits[p], stages)
        for t in range(pl.n):
            if xs[p][t] is None:
                continue
            coef = sm.coef[p, t].copy()
            c16 = torch.from_numpy(coef[:k]).half().numpy()
            assert np.array_equal(sm.c_high[p, t, :k].view(np.uint16), c16.view(np.uint16)), (p, t)
            if nl == 0:
                continue
            got = {"codes": sm.codes[p, t, :, :nl], "scale": sm.scale[p, t], "zero_point": sm.zero_point[p, t],
                   "residual_norm": sm.residual_norm[p, t]}
            want_c = orc.rtvq_quantize(coef[k:r], pl.bits[p], stages)
            pays = quant.quantize(torch.from_numpy(coef[k:r].copy()))["payloads"]
            want_q = {"codes": np.stack([q["quantized"].numpy() for q in pays]),
                      "scale": np.array([float(q["scale"]) for q in pays], np.float32),
                      "zero_point": np.array([float(q["zero_point"]) for q in pays], np.float32),
                      "residual_norm": np.array([q["residual_norm"] for q in pays], np.float32)}
            for who, want in (("C oracle", want_c), ("RTVQQuantizer", want_q)):
                assert np.array_equal(got["codes"], want["codes"]), (who, p, t)
                for f in ("scale", "zero_point", "residual_norm"):
                    assert same_bits(got[f], want[f]), (who, f, p, t, got[f], want[f])


@pytest.mark.parametrize("stages", [1, 2, 4])
@pytest.mark.parametrize("bits", [1, 4, 8, "mixed"])
def test_epilogue_is_the_quantizer_on_the_kernels_coefficients(sq, orc, bits, stages):
    params = [(255, "k0"), (256, "k=r"), (257, "r<N"), (1027, "r=N")]
    b = [8, 2, 1, 5] if bits == "mixed" else bits
    pl = Plan(sq, 8, fp16=True, center=True, params=params, bits=b, stages=stages)
    xs = _inputs(pl, seed=3)
    sm = pl.plan.project_tasks(pl.table(_cuda(xs)))
    _assert_epilogue(sq, orc, pl, sm, xs, stages)


def test_epilogue_above_16_tasks(sq, orc):
    pl = Plan(sq, 20, fp16=False, center=False, params=[(257, "r<N"), (1027, "r=N")])
    xs = _inputs(pl, seed=4)
    sm = pl.plan.project_tasks(pl.table(_cuda(xs)))
    _assert_epilogue(sq, orc, pl, sm, xs, 2)


# ------------------------------------------------------------------------------------------ 5. slots, bounds, determinism
def _writable(pl, present):
    """Byte mask over the small buffer: what a projection of the `present` (p, t) slots may write."""
    L, n, S = pl.plan.layout, pl.n, pl.plan.S
    m = np.zeros(int(L.total_bytes), dtype=bool)
    for p, t in present:
        slot = p * n + t
        m[L.chigh_off + slot * n * 2:L.chigh_off + (slot + 1) * n * 2] = True
        m[L.coef_off + slot * n * 4:L.coef_off + (slot + 1) * n * 4] = True
        m[L.codes_off + slot * S * n:L.codes_off + (slot + 1) * S * n] = True
        for off in (L.scale_off, L.zp_off, L.rnorm_off):
            m[off + slot * S * 4:off + (slot + 1) * S * 4] = True
    return m


@pytest.mark.parametrize("n", [3, 8, 20])
def test_null_slots_guards_and_determinism(sq, n):
    pl = Plan(sq, n, fp16=True, center=True)
    absent = {(p, t) for p in range(len(pl.rows)) for t in range(n) if (p + t) % 3 == 1}
    absent |= {(2, t) for t in range(n)}          # a parameter none of whose slots is present
    xs = _inputs(pl, seed=7, absent=absent)
    present = [(p, t) for p, rows in enumerate(pl.rows) if rows > 0 for t in range(n) if (p, t) not in absent]
    whole = pl.plan.basis._base                    # basis, the gap behind it and the mean: one allocation
    assert whole is not None and whole.numel() >= pl.plan.basis.numel() + pl.plan.mean.numel() * 4
    before_basis, before_small = whole.cpu().numpy().copy(), pl.small_bytes()
    tab = pl.table(_cuda(xs))
    sm = pl.plan.project_tasks(tab, rows_dev=pl.rows_dev)
    after1 = pl.small_bytes()
    assert np.array_equal(whole.cpu().numpy(), before_basis)          # the basis and the mean are only read
    keep = ~_writable(pl, present)
    assert np.array_equal(after1[keep], before_small[keep])           # sigma, k, r, energy, rows, absent slots, padding
    assert (before_small[pl.plan.layout.chigh_off:pl.plan.layout.status_off] == SENTINEL).all()
    _assert_truth(pl, sm, xs)
    for p, t in present:                                               # a present slot is written, not left as it was
        assert not (sm.coef[p, t].view(np.uint8) == SENTINEL).all()
    # the same call again, and on a fresh plan: identical bytes
    pl.plan.project_tasks(tab, rows_dev=pl.rows_dev)
    assert np.array_equal(pl.small_bytes(), after1)
    again = Plan(sq, n, fp16=True, center=True)
    again.plan.project_tasks(again.table(_cuda(xs)), rows_dev=again.rows_dev)
    assert np.array_equal(again.small_bytes(), after1)


def test_refusals_write_nothing(sq):
    from ctypes import c_void_p
    from svdq_amd import _native as nat
    pl = Plan(sq, 8, fp16=True, center=True, params=[(257, "r<N")])
    xs = _inputs(pl)
    tab = pl.table(_cuda(xs))
    plan, lib = pl.plan, nat.lib()
    work = torch.empty(int(lib.svdq_plan_project_work_bytes(plan._h)), dtype=torch.uint8, device=pl.dev)
    assert work.numel() >= plan.sizes.n_units * 8 * 8 * 8
    before = pl.small_bytes()
    good = dict(plan=plan._h, table=tab.data_ptr(), basis=plan.basis.data_ptr(), mean=plan.mean.data_ptr(),
                small=plan.small.data_ptr(), work=work.data_ptr())
    for missing in ("plan", "table", "basis", "mean", "small", "work"):
        a = dict(good)
        a[missing] = None
        rc = lib.svdq_plan_project(a["plan"], c_void_p(a["table"]), None, None, None, c_void_p(a["basis"]),
                                   c_void_p(a["mean"]), c_void_p(a["small"]), c_void_p(a["work"]), None)
        assert rc == nat.SVDQ_EINVAL, missing
        assert "svdq_plan_project" in nat.last_error(), missing
    torch.cuda.synchronize()
    assert np.array_equal(pl.small_bytes(), before)
    # the host layer refuses tables whose sizes disagree with the plan
    with pytest.raises(ValueError, match="svdq_plan_project"):
        plan.project_tasks(tab[:-1].contiguous())
    with pytest.raises(ValueError, match="svdq_plan_project"):
        plan.project_tasks(tab, base_table=torch.zeros(2, dtype=torch.int64, device=pl.dev))
    assert np.array_equal(pl.small_bytes(), before)


# ------------------------------------------------------------------------------------------ 6. against the fused route
@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
def test_against_the_fused_route(sq, orc, fp16):
    """8 tasks through svdq_compress, then the same deltas projected onto the plan's own (rounded) basis: the two sets of
    coefficients agree within the tolerance tests/test_hip_parity.py holds the per-call projection to, and both sit
    inside bound 1 of the fp64 truth."""
    n, rows = 8, [1027, 4099]
    dev = torch.device("cuda", 0)
    deltas = [orc.synthetic_deltas(r, n, seed=11 + r) for r in rows]
    vs = [[d.to(dev) for d in ds] for ds in deltas]
    plan, sm = sq.compress_batch(vs, energy_threshold=0.9, max_rank=None, center=True, fp16=fp16, low_bits=4,
                                 rtvq_stages=2, device=dev, unit_rows=256)
    fused = sm.coef.copy()
    table = plan.pointer_table(vs)
    sm2 = plan.project_tasks(table)
    for f in ("sigma", "k", "r", "energy", "rows"):
        assert np.array_equal(getattr(sm2, f), getattr(sm, f)), f
    for p, r_ in enumerate(rows):
        k, r = int(sm.k[p]), int(sm.r[p])
        U_high, U_low, mean = plan.basis_tensors(p, k, r, r_)
        u = torch.cat([U_high, U_low], dim=1).double().cpu()
        m = mean.reshape(-1).cpu()
        for t in range(n):
            xc = (deltas[p][t].float() - m)
            ref, mag = u.T @ xc.double(), u.abs().T @ xc.double().abs()
            bound = 258 * U * mag + U * ref.abs()
            for who, c in (("projected", sm2.coef[p, t, :r]), ("fused", fused[p, t, :r])):
                err = (torch.from_numpy(c.copy()).double() - ref).abs()
                assert bool((err <= bound).all()), (who, p, t, float((err / bound).max()))
            np.testing.assert_allclose(sm2.coef[p, t, :r], fused[p, t, :r], rtol=2e-4, atol=1e-6)
