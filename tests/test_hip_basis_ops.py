"""
The caller-basis kernels of csrc/svdq_basis_ops.hip -- k_project, k_reconstruct, k_recon_error and their finish kernels
-- through the C ABI with raw pointers (``svdq_project``, ``svdq_reconstruct``, ``svdq_recon_error``; no Python wrapper
converts anything), against the fp64 model and the derived bounds of tests/basis_ops_model.py, at the row counts where
THEIR geometry changes: a thread's second row (257), the second block (2049), a third (4097), and the ninth row per
thread past 1024 * 2048.  Every (k, nl) with k + nl <= 4 and the wide pairs up to 32 columns, both basis types, the
mean present and absent, the fused and the given-reconstruction forms, NaN and Inf operands, refusals, determinism, and
sentinel bytes around every output.
"""
import numpy as np
import pytest
import torch

import basis_ops_model as bm
from helpers import diag_check, diag_check_given

pytestmark = pytest.mark.gpu

GUARD = 256          # bytes of sentinel on each side of an output
SENTINEL = 0xA5
HEADROOM = {}        # operator -> worst error / bound seen (a measurement, printed; nothing asserts it)


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from svdq_amd import _native
    return _native.lib()


class Guarded:
    """``count`` elements of ``dtype`` on the device between two runs of sentinel bytes."""

    def __init__(self, count, dtype):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        pad = (self.nbytes + 15) // 16 * 16
        self.raw = torch.full((GUARD + pad + GUARD,), SENTINEL, dtype=torch.uint8, device=_dev())
        self.data = self.raw[GUARD:GUARD + self.nbytes].view(dtype)

    def ptr(self):
        return self.data.data_ptr()

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == SENTINEL).all()) and bool((r[GUARD + self.nbytes:] == SENTINEL).all())

    def untouched(self):
        return bool((self.raw == SENTINEL).all())


class Operands:
    """One model case on the device."""

    def __init__(self, c):
        d = _dev()
        self.c = c
        self.uh = c.U_high.to(d) if c.k else None
        self.ul = c.U_low.to(d) if c.nl else None
        self.coef, self.mean, self.orig, self.delta = c.coef.to(d), c.mean.to(d), c.orig.to(d), c.delta.to(d)


_OPS = {}


def _operands(rows, k, nl, fp16):
    key = (rows, k, nl, fp16)
    if key not in _OPS:
        if rows > 100000:      # the two long cases: keep one basis on the device at a time
            _OPS.clear()
        _OPS[key] = Operands(bm.Case(rows, k, nl, fp16))
    return _OPS[key]


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _note(op, ratio):
    HEADROOM[op] = max(HEADROOM.get(op, 0.0), float(ratio))


def project(lib, o, use_mean, k=None, nl=None):
    c = o.c
    k, nl = (c.k, c.nl) if k is None else (k, nl)
    out = Guarded(max(k + nl, 1), torch.float32)
    work = Guarded(int(lib.svdq_project_work_bytes(c.rows, k + nl)), torch.uint8)
    rc = lib.svdq_project(_p(o.uh), _p(o.ul), int(c.fp16), c.rows, k, nl, _p(o.delta), _p(o.mean) if use_mean else None,
                          out.ptr(), work.ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out, work


def reconstruct(lib, o, use_mean, scale, k=None, nl=None):
    c = o.c
    k, nl = (c.k, c.nl) if k is None else (k, nl)
    out = Guarded(c.rows, torch.float32)
    rc = lib.svdq_reconstruct(_p(o.uh), _p(o.ul), int(c.fp16), c.rows, k, nl, _p(o.coef) if k + nl else None,
                              _p(o.mean) if use_mean else None, float(scale), out.ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


def recon_error(lib, o, use_mean, recon=None, orig=None, k=None, nl=None):
    c = o.c
    k, nl = (c.k, c.nl) if k is None else (k, nl)
    out = Guarded(6, torch.float64)
    work = Guarded(int(lib.svdq_recon_error_work_bytes(c.rows)), torch.uint8)
    x = o.orig if orig is None else orig
    if recon is None:
        rc = lib.svdq_recon_error(_p(o.uh), _p(o.ul), int(c.fp16), c.rows, k, nl, _p(o.coef), _p(o.mean) if use_mean else None,
                                  None, _p(x), out.ptr(), work.ptr(), _stream())
    else:
        rc = lib.svdq_recon_error(None, None, 0, c.rows, 0, 0, None, None, _p(recon), _p(x), out.ptr(), work.ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out, work


def _six(out):
    return dict(zip(bm.KEYS, out.data.cpu().tolist()))


def _check_case(lib, o):
    """All three operators on one case: mean present and absent, scale 1 and 0.5, fused and given forms."""
    c = o.c
    what = (c.rows, c.k, c.nl, "fp16" if c.fp16 else "fp32")
    for use_mean in (False, True):
        mean = c.mean if use_mean else None
        rc, out, work = project(lib, o, use_mean)
        assert rc == 0 and out.guards_intact() and work.guards_intact(), (what, "project", rc)
        want, bound = bm.project_exact(c.U_high, c.U_low, c.delta, mean)
        err = (out.data.cpu().double() - want).abs()
        _note("project", float((err / bound).max()))
        assert bool((err <= bound).all()), (what, "project", use_mean, float((err / bound).max()))
        for scale in (1.0, 0.5):
            rc, out = reconstruct(lib, o, use_mean, scale)
            assert rc == 0 and out.guards_intact(), (what, "reconstruct", rc)
            want, bound = bm.reconstruct_exact(c.U_high, c.U_low, c.coef, mean, scale)
            err = (out.data.cpu().double() - want).abs()
            _note("reconstruct", float((err / (bound + 1e-300)).max()))
            assert bool((err <= bound).all()), (what, "reconstruct", use_mean, scale, int((err / (bound + 1e-300)).argmax()))
        rc, out, work = recon_error(lib, o, use_mean)
        assert rc == 0 and out.guards_intact() and work.guards_intact(), (what, "recon_error", rc)
        got = _six(out)
        _note("recon_error", max(bm.six_ratio(got, c.orig, c.U_high, c.U_low, c.c_high(), c.c_low(), mean=mean).values()))
        diag_check(got, c.orig, c.U_high, c.U_low, c.c_high(), c.c_low(), what=(what, "fused", use_mean), mean=mean)
    # the given-reconstruction form: the basis is not read (its arguments are null)
    rec = (c.orig + 0.3 * c.delta).contiguous()
    rc, out, work = recon_error(lib, o, False, recon=rec.to(_dev()))
    assert rc == 0 and out.guards_intact() and work.guards_intact(), (what, "recon_error given", rc)
    got = _six(out)
    _note("recon_error_given", max(bm.six_ratio(got, c.orig, None, None, None, None, recon=rec).values()))
    diag_check_given(got, c.orig, rec, what=(what, "given"))


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rows", bm.ROWS)
def test_three_operators_against_fp64(lib, rows, fp16):
    for k, nl in bm.PAIRS:
        _check_case(lib, _operands(rows, k, nl, fp16))
    print("worst error / bound so far:", {k: round(v, 4) for k, v in HEADROOM.items()})


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rows", bm.ROWS_HUGE)
def test_the_ninth_row_of_a_thread(lib, rows, fp16):
    """1024 * 2048 rows: the grid is at its cap and every thread visits 8 rows; one row more and thread 0 visits a ninth.
    k + nl <= 2 only: the fp16 basis is 8 MB."""
    assert bm.rows_per_thread(rows) == (8 if rows == bm.ROWS_HUGE[0] else 9)
    for k, nl in [p for p in bm.PAIRS_SMALL if sum(p) <= 2]:
        _check_case(lib, _operands(rows, k, nl, fp16))
    _OPS.clear()
    print("worst error / bound so far:", {k: round(v, 4) for k, v in HEADROOM.items()})


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rows", [1, 257, 4097])
def test_reconstruct_without_columns(lib, rows, fp16):
    """k + nl = 0: ``mean * scale`` exactly, or zeros."""
    o = _operands(rows, 1, 1, fp16)
    for scale in (1.0, 0.5):
        rc, out = reconstruct(lib, o, True, scale, k=0, nl=0)
        assert rc == 0 and out.guards_intact()
        assert np.array_equal(out.data.cpu().numpy().view(np.uint32), (o.c.mean.numpy() * np.float32(scale)).view(np.uint32))
        rc, out = reconstruct(lib, o, False, scale, k=0, nl=0)
        assert rc == 0 and out.guards_intact()
        assert np.array_equal(out.data.cpu().numpy().view(np.uint32), np.zeros(rows, np.uint32))


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
def test_refusals_write_nothing(lib, fp16):
    """k + nl = 33 on all three and k + nl = 0 on the projection: SVDQ_EINVAL, and not a byte of the outputs or the
    workspace is written."""
    from svdq_amd import _native
    o = _operands(257, 2, 2, fp16)
    for k, nl in ((33, 0), (0, 33), (16, 17), (1, 32)):
        rc, out, work = project(lib, o, True, k=k, nl=nl)
        assert rc == _native.SVDQ_EINVAL and out.untouched() and work.untouched(), ("project", k, nl, rc)
        rc, out = reconstruct(lib, o, True, 0.5, k=k, nl=nl)
        assert rc == _native.SVDQ_EINVAL and out.untouched(), ("reconstruct", k, nl, rc)
        rc, out, work = recon_error(lib, o, True, k=k, nl=nl)
        assert rc == _native.SVDQ_EINVAL and out.untouched() and work.untouched(), ("recon_error", k, nl, rc)
    rc, out, work = project(lib, o, True, k=0, nl=0)
    assert rc == _native.SVDQ_EINVAL and out.untouched() and work.untouched()
    assert "k + nl" in _native.last_error()


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rows", [2048, 4097])
def test_nonfinite_operands_have_torchs_pattern(lib, rows, fp16):
    """One NaN at row 0, 256, the middle or the last row -- in ``orig`` for the fused form, in the reconstruction for the
    given form -- and, separately, one +Inf in ``orig``: each of the six numbers is NaN / Inf exactly where torch's is,
    and the finite ones stay inside the bound.  (``max_absolute_error`` used to keep a NaN only when it sat in the last
    row a thread visits: finite beside a NaN ``absolute_error`` at rows 0, 256 and the middle.)"""
    o = _operands(rows, 2, 2, fp16)
    c = o.c
    rec = (c.orig + 0.3 * c.delta).contiguous()
    for value, at in [(float("nan"), r) for r in (0, 256, rows // 2, rows - 1)] + [(float("inf"), 256)]:
        x = c.orig.clone()
        x[at] = value
        for use_mean in (False, True):
            rc, out, work = recon_error(lib, o, use_mean, orig=x.to(_dev()))
            assert rc == 0 and out.guards_intact() and work.guards_intact()
            print("fused", rows, value, at, use_mean, _six(out))
            bm.check_six_nonfinite(_six(out), x, c.U_high, c.U_low, c.c_high(), c.c_low(),
                                   mean=c.mean if use_mean else None, what=("fused", rows, value, at, use_mean))
        bad = rec.clone()
        given_x = c.orig
        if value != value:
            bad[at] = value      # the NaN sits in the reconstruction
        else:
            given_x = x          # the Inf sits in orig
        rc, out, work = recon_error(lib, o, False, recon=bad.to(_dev()), orig=given_x.to(_dev()))
        assert rc == 0 and out.guards_intact() and work.guards_intact()
        print("given", rows, value, at, _six(out))
        bm.check_six_nonfinite(_six(out), given_x, None, None, None, None, recon=bad, what=("given", rows, value, at))


def test_two_runs_give_identical_bits(lib):
    for fp16 in (True, False):
        o = _operands(4097, 7, 9, fp16)
        a, b = [], []
        for got in (a, b):
            got.append(project(lib, o, True)[1].data.cpu().numpy().view(np.uint32))
            got.append(reconstruct(lib, o, True, 0.5)[1].data.cpu().numpy().view(np.uint32))
            got.append(recon_error(lib, o, True)[1].data.cpu().numpy().view(np.uint64))
            got.append(recon_error(lib, o, False, recon=o.delta)[1].data.cpu().numpy().view(np.uint64))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ pinned bits
def dyadic_operands(rows, k, nl, fp16):
    """Operands made of small dyadic rationals by integer arithmetic: the same bits on every machine and every version
    of torch, so the six numbers of a finite case can be pinned as bit patterns."""
    d = torch.arange(rows, dtype=torch.int64)
    r = k + nl
    U = (((d[:, None] * 37 + torch.arange(r)[None, :] * 11) % 101) - 50).double() / 64.0
    c = bm.Case.__new__(bm.Case)
    c.rows, c.k, c.nl, c.r, c.fp16 = rows, k, nl, r, fp16
    dt = torch.float16 if fp16 else torch.float32
    c.U_high, c.U_low = U[:, :k].to(dt).contiguous(), U[:, k:].to(dt).contiguous()
    c.coef = ((torch.arange(r) * 7 % 13) - 6).float() / 8.0
    c.mean = (((d * 13) % 29) - 14).float() / 256.0
    c.orig = (((d * 53) % 97) - 48).float() / 32.0
    c.delta = (((d * 29) % 89) - 44).float() / 32.0
    return Operands(c)


# svdq_recon_error on finite operands returns the bits it returned before max_absolute_error learnt to keep a NaN
# (the change moved the NaN test from the row loop to the finish kernel): the six float64 results of two cases as the
# build before that change gave them on an MI355X
PINNED = {
    (4097, 7, 9, True, True): ["405106cb80000000", "3ff373a846583af5", "40073c0000000000", "3fec218ae0000000",
                               "404c029fa0000000", "404360e520000000"],
    (2049, 2, 2, False, False): ["4045f26900000000", "3ff1b907913e4a9c", "4002ac0000000000", "3fea1145e0000000",
                                 "4043d04360000000", "403311d4a0000000"],
}


@pytest.mark.parametrize("key", sorted(PINNED), ids=lambda k: "rows%d-k%d-nl%d-%s-%s" % (
    k[0], k[1], k[2], "fp16" if k[3] else "fp32", "mean" if k[4] else "nomean"))
def test_finite_results_keep_their_bits(lib, key):
    rows, k, nl, fp16, use_mean = key
    o = dyadic_operands(rows, k, nl, fp16)
    rc, out, work = recon_error(lib, o, use_mean)
    assert rc == 0
    got = ["%016x" % v for v in out.data.cpu().numpy().view(np.uint64).tolist()]
    print("recon_error bits", key, got)
    c = o.c
    diag_check(_six(out), c.orig, c.U_high, c.U_low, c.c_high(), c.c_low(), what=key, mean=c.mean if use_mean else None)
    assert got == PINNED[key]
