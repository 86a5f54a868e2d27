"""
The input side of csrc/svdq_torch.cpp: the preparation branches (``prep``, ``prep_in``, ``input_type_of``, ``mask_bytes``,
``basis_args``) under every form a caller's tensor can take, ``mask_select`` over dtypes, masks and shapes, the quantizer
operators over lengths, widths and stage counts, and the caller-basis operators ``reconstruct`` / ``recon_error`` against
the fp64 model of tests/basis_ops_model.py -- mixed element types included: a basis array is never rounded down to its
neighbour's type.
"""
import numpy as np
import pytest
import torch

import basis_ops_model as bm
from helpers import bits_equal, diag_check
from torch_ops_layer import Settings, dev, reference, reference_regions, regions, same, same_bits

pytestmark = pytest.mark.gpu
OPS = None


@pytest.fixture(scope="module", autouse=True)
def _ops_loaded():
    global OPS
    import svdq_amd  # noqa: F401
    from svdq_amd import torch_ops
    torch_ops.load()
    OPS = torch.ops.svdq


# ------------------------------------------------------------------------------------------------ 4. input forms
FORM_ROWS = [264, 4104]      # multiples of 24: every form below can shape them
N_FORM = 8      # enough tasks for a finite store: at 2 or 3 the one-column quantizer range is degenerate (NaN)
MAX_STAGES = 8  # SVDQ_MAX_STAGES of include/svdq.h


def _offset(v):
    buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=v.device)
    buf[1:] = v
    return buf[1:]      # 4 bytes (fp32) or 2 bytes (half) off the allocation's alignment: the clone branches


FORMS = {
    # name: (canonical fp32 values of v, the tensor handed to the operator)
    "transposed": (lambda v: v, lambda v: v.view(v.numel() // 12, 12).t().contiguous().t()),
    "offset": (lambda v: v, _offset),
    "4d": (lambda v: v, lambda v: v.view(2, 3, 4, v.numel() // 24)),
    "requires_grad": (lambda v: v, lambda v: v.clone().requires_grad_(True)),
    "float64": (lambda v: v, lambda v: v.double()),
    "fp16": (lambda v: v.half().float(), lambda v: v.half()),
    "bf16": (lambda v: v.bfloat16().float(), lambda v: v.bfloat16()),
    "fp16_offset": (lambda v: v.half().float(), lambda v: _offset(v.half())),
    "bf16_transposed": (lambda v: v.bfloat16().float(), lambda v: v.bfloat16().view(v.numel() // 12, 12).t().contiguous().t()),
    "mixed": None,      # one fp16 tensor among fp32 ones: the fallback to fp32
}


def _forms(name, tensors):
    """(canonical fp32 clones, the same values in form ``name``) of a list of flat fp32 tensors."""
    if name == "mixed":
        canon = [tensors[0].half().float()] + [t.clone() for t in tensors[1:]]
        return canon, [tensors[0].half()] + [t.clone() for t in tensors[1:]]
    c, f = FORMS[name]
    canon = [c(t).contiguous().clone() for t in tensors]
    formed = [f(t) for t in tensors]
    for a, b in zip(canon, formed):      # the form holds the canonical values, in the canonical order
        assert torch.equal(b.detach().float().contiguous().view(-1), a)
    return canon, formed


@pytest.mark.parametrize("name", list(FORMS))
def test_every_input_form_gives_the_canonical_bits(name):
    """compress, compress_from_base, task_gram, diagnostics, ingest, rtvq_quantize and mask_select on a transposed view,
    a misaligned view, a 4-D tensor, a tensor that requires grad, float64, all-fp16, all-bf16 and one fp16 among fp32:
    bit for bit the operator on canonical fp32 clones (the native half forms also against the half-input ctypes route)."""
    from oracle import svd_hybrid_oracle as orc
    st, n, rows = Settings(), N_FORM, FORM_ROWS
    g = torch.Generator().manual_seed(77)
    raw = [d.to(dev()) for D in rows for d in orc.synthetic_deltas(D, n, 500 + D)]
    braw = [(0.5 * torch.randn(D, generator=g)).to(dev()) for D in rows]
    canon, formed = _forms(name, raw)
    bcanon, bformed = _forms(name, braw) if name != "mixed" else ([b.clone() for b in braw], [b.clone() for b in braw])
    lay = st.plan(rows, n, gram_only=True)
    # compress
    want = OPS.compress(canon, n, *st.args())
    got = OPS.compress(formed, n, *st.args())
    assert same(regions(lay, *got), regions(lay, *want)), name
    if name in ("fp16", "bf16"):      # the kernels read the half tensors as they are: the half-input ctypes route
        vecs = [formed[p * n:(p + 1) * n] for p in range(len(rows))]
        ref = reference(rows, n, vecs, st, input_dtype=formed[0].dtype)
        assert same(regions(lay, *got), reference_regions(ref)), name
    # diagnostics of the canonical store against the formed deltas
    d_want = OPS.diagnostics(canon, [], *want, n, *st.args(), False)
    d_got = OPS.diagnostics(formed, [], *want, n, *st.args(), False)
    assert same_bits(d_got, d_want) and bool(torch.isfinite(d_want).all()), name
    # task_gram
    assert same_bits(OPS.task_gram(formed, n), OPS.task_gram(canon, n)), name
    # compress_from_base: fine-tuned = base + delta, formed like the deltas
    ft_raw = [braw[p] + raw[p * n + t] for p in range(len(rows)) for t in range(n)]
    fcanon, fformed = _forms(name, ft_raw)
    want_b = OPS.compress_from_base(fcanon, bcanon, n, *st.args())
    got_b = OPS.compress_from_base(fformed, bformed, n, *st.args())
    assert same(regions(lay, *got_b), regions(lay, *want_b)), name
    # ingest: the result takes the base tensor's shape
    outs_want = OPS.ingest(bcanon[0], fcanon[:n])
    outs_got = OPS.ingest(bformed[0], fformed[:n])
    for a, b, f in zip(outs_got, outs_want, fcanon[:n]):
        assert a.shape == bformed[0].shape and a.dtype == torch.float32
        assert torch.equal(a.reshape(-1), b.reshape(-1)) and torch.equal(b.reshape(-1), f - bcanon[0]), name
    # rtvq_quantize
    q_want = OPS.rtvq_quantize(canon[0], 4, 2)
    q_got = OPS.rtvq_quantize(formed[0], 4, 2)
    assert same(q_got, q_want), name
    # mask_select keeps the dtype and the values
    mask = (torch.rand(rows[0], generator=g) < 0.5).to(dev())
    x = formed[0]      # as formed: a tensor that requires grad reaches the operator's own detach
    sel = OPS.mask_select(x, mask.view(x.shape), False)      # both are read in the contiguous order of their shape
    assert sel.dtype == x.dtype and torch.equal(sel.detach().float(), canon[0][mask]), name


# ------------------------------------------------------------------------------------------------ 7. mask_select
SELECT_DTYPES = [torch.bool, torch.uint8, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32,
                 torch.float64]
SHAPE3 = {1: (1, 1, 1), 7: (7, 1, 1), 8: (2, 2, 2), 9: (3, 1, 3), 5000: (10, 20, 25)}


def _values(dtype, n, g):
    if dtype is torch.bool:
        return torch.rand(n, generator=g) < 0.5
    if dtype is torch.uint8:
        return torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    if dtype is torch.int32:
        x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g).to(torch.int32)
        x[0] = 2 ** 24 + 1
        return x
    if dtype is torch.int64:
        x = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g)
        special = torch.tensor([2 ** 24 + 1, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -2 ** 63])
        x[:min(n, 5)] = special[:min(n, 5)]
        return x
    if dtype is torch.float64:
        x = torch.randn(n, generator=g, dtype=torch.float64)
        special = torch.tensor([1.0 + 2.0 ** -40, 1e-300, -1e300], dtype=torch.float64)
        x[:min(n, 3)] = special[:min(n, 3)]
        return x
    return torch.randn(n, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", SELECT_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_mask_select_is_exact_for_every_dtype(dtype):
    """``x[mask]`` / ``x[~mask]`` exactly, in x's dtype: int64 values past 2^24 and 2^53 and float64 values fp32 cannot
    hold come back as they went in (every non-fp32 dtype used to travel through fp32 and back)."""
    g = torch.Generator().manual_seed(3)
    for n in (1, 7, 8, 9, 5000):
        vals = _values(dtype, n, g)
        for kind in ("random", "all", "none"):
            m = {"random": torch.rand(n, generator=g) < 0.5, "all": torch.ones(n, dtype=torch.bool),
                 "none": torch.zeros(n, dtype=torch.bool)}[kind]
            s3 = SHAPE3[n]
            big = torch.zeros(s3[0], s3[1], 2 * s3[2], dtype=dtype)
            big[:, :, ::2] = vals.view(s3)
            x3 = big.to(dev())[:, :, ::2]      # 3-D, not contiguous
            assert n == 1 or not x3.is_contiguous()
            for x, mask in ((vals.to(dev()), m.to(dev())), (x3, m.view(s3).to(dev()))):
                for invert in (False, True):
                    got = OPS.mask_select(x, mask, invert)
                    want = x[~mask] if invert else x[mask]
                    assert got.dtype == dtype and got.shape == want.shape, (dtype, n, kind, invert)
                    assert torch.equal(got, want), (dtype, n, kind, invert)
    # a uint8 mask is read as it is
    x, m = _values(dtype, 9, g).to(dev()), (torch.arange(9) % 2).to(torch.uint8).to(dev())
    assert torch.equal(OPS.mask_select(x, m, False), x[m.bool()])


def test_mask_select_refusals():
    x = torch.randn(8, device=dev())
    with pytest.raises(ValueError, match="Shape mismatch"):
        OPS.mask_select(x, torch.ones(7, dtype=torch.bool, device=dev()), False)
    with pytest.raises(ValueError, match="mask_select: dtype ComplexFloat"):      # named, never rounded
        OPS.mask_select(x.to(torch.complex64), torch.ones(8, dtype=torch.bool, device=dev()), False)
    assert OPS.mask_select(x[:0], torch.ones(0, dtype=torch.bool, device=dev()), False).numel() == 0


def test_mask_combine_and_indices_refusals():
    d = dev()
    a, b = torch.ones(8, dtype=torch.bool, device=d), torch.ones(7, dtype=torch.bool, device=d)
    for bad, fragment in [
        (lambda: OPS.mask_combine([a, a], "xor"), "Unknown mask strategy"),
        (lambda: OPS.mask_combine([a, b], "union"), "Shape mismatch"),
        (lambda: OPS.mask_combine([a, a.cpu()], "union"), "all masks must live on one device"),
        (lambda: OPS.mask_combine_indices([a, a], 0, "union"), "Empty mask list"),
        (lambda: OPS.mask_combine_indices([a, a, a], 2, "union"), "n_masks masks per parameter"),
        (lambda: OPS.mask_combine_indices([a, a], 2, "xor"), "Unknown mask strategy"),
        (lambda: OPS.mask_combine_indices([a[:0], a[:0]], 2, "union"), "empty mask"),
        (lambda: OPS.mask_combine_indices([a, a.cpu()], 2, "union"), "all masks must live on one device"),
        (lambda: OPS.mask_combine_indices([a, b], 2, "union"), "Shape mismatch"),
    ]:
        with pytest.raises(ValueError, match=fragment):
            bad()
    # masks of another dtype are taken as their truth values; a uint8 mask as it is
    f = torch.tensor([0.0, 2.0, 0.0, -1.0], device=d)
    u = torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=d)
    assert torch.equal(OPS.mask_combine([f, u], "intersection"), torch.tensor([False, False, False, True], device=d))


# ------------------------------------------------------------------------------------------------ 8. quantizer operators
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097]


@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_quantizer_operators_against_the_oracle(bits):
    from oracle import svd_hybrid_oracle as orc
    g = torch.Generator().manual_seed(bits)
    for n in LENGTHS:
        x = (0.02 * torch.randn(n, generator=g)).to(dev())
        for stages in range(1, MAX_STAGES + 1):
            codes, scale, zp, rn = OPS.rtvq_quantize(x, bits, stages)
            want = orc.rtvq_quantize(x.cpu().numpy(), bits, stages)
            what = (bits, n, stages)
            assert codes.shape == (stages, n) and np.array_equal(codes.cpu().numpy(), want["codes"]), what
            assert bits_equal(scale.cpu().numpy(), want["scale"]) and bits_equal(zp.cpu().numpy(), want["zero_point"]), what
            np.testing.assert_allclose(rn.cpu().numpy(), want["residual_norm"], rtol=1e-5, equal_nan=True)
            truth = orc.rtvq_dequantize(want).reshape(-1)
            assert bits_equal(OPS.rtvq_dequantize(codes, scale, zp).cpu().numpy(), truth), what
            if stages in (1, 3):
                # CPU scale / zero point; a column slice of a wider code array; codes one byte off their alignment
                assert bits_equal(OPS.rtvq_dequantize(codes, scale.cpu(), zp.cpu()).cpu().numpy(), truth), what
                wide = torch.zeros(stages, n + 8, dtype=torch.uint8, device=dev())
                wide[:, 3:3 + n] = codes
                sl = wide[:, 3:3 + n]
                assert stages == 1 or not sl.is_contiguous()
                assert bits_equal(OPS.rtvq_dequantize(sl, scale, zp).cpu().numpy(), truth), what
                off = torch.zeros(stages * n + 1, dtype=torch.uint8, device=dev())
                off[1:] = codes.reshape(-1)
                assert bits_equal(OPS.rtvq_dequantize(off[1:].view(stages, n), scale, zp).cpu().numpy(), truth), what
            if stages == 1:      # 1-D codes are one stage
                assert bits_equal(OPS.rtvq_dequantize(codes[0], scale, zp).cpu().numpy(), truth), what


def test_quantizer_operator_refusals_and_empty_input():
    x = torch.randn(16, device=dev())
    for bad, fragment in [
        (lambda: OPS.rtvq_quantize(x, 0, 2), "bits in"),
        (lambda: OPS.rtvq_quantize(x, 9, 2), "bits in"),
        (lambda: OPS.rtvq_quantize(x, 4, 0), "stages out of range"),
        (lambda: OPS.rtvq_quantize(x, 4, MAX_STAGES + 1), "stages out of range"),
        (lambda: OPS.rtvq_quantize(x[:0], 4, 2), "empty tensor"),
        (lambda: OPS.rtvq_dequantize(torch.zeros(2, 4, dtype=torch.int32, device=dev()), x[:2], x[:2]), "codes are uint8"),
        (lambda: OPS.rtvq_dequantize(torch.zeros(2, 2, 4, dtype=torch.uint8, device=dev()), x[:2], x[:2]), "codes are uint8"),
        (lambda: OPS.rtvq_dequantize(torch.zeros(2, 4, dtype=torch.uint8, device=dev()), x[:3], x[:2]),
         "one scale / zero point per stage"),
    ]:
        with pytest.raises(ValueError, match=fragment):
            bad()
    out = OPS.rtvq_dequantize(torch.zeros(2, 0, dtype=torch.uint8, device=dev()), x[:2], x[:2])      # n = 0
    assert out.numel() == 0 and out.dtype == torch.float32
    base = torch.randn(6, device=dev())
    with pytest.raises(ValueError, match="no fine-tuned tensors"):
        OPS.ingest(base, [])
    with pytest.raises(ValueError, match="differ in size"):
        OPS.ingest(base, [base[:5]])
    assert [o.shape for o in OPS.ingest(base[:0].view(0, 3), [base[:0]])] == [(0, 3)]


# ------------------------------------------------------------------------------------------------ 9. caller-basis operators
def _on(c, high=None, low=None):
    """The case's basis on the device, each array in its own element type."""
    d = dev()
    Uh = c.U_high.to(d) if high is None else c.U_high.to(high).to(d)
    Ul = c.U_low.to(d) if low is None else c.U_low.to(low).to(d)
    return Uh, Ul


def _check_ops(c, Uh, Ul, what):
    """reconstruct (scale 1 and 0.5) and recon_error, mean a tensor or None, against the model on the tensors AS GIVEN."""
    d = dev()
    Uh_c, Ul_c = Uh.cpu(), Ul.cpu()
    coef, orig = c.coef.to(d), c.orig.to(d)
    for mean in (None, c.mean):
        mdev = None if mean is None else mean.to(d)
        for scale in (1.0, 0.5):
            out = OPS.reconstruct(Uh, Ul, coef, mdev, scale)
            want, bound = bm.reconstruct_exact(Uh_c, Ul_c, c.coef, mean, scale)
            err = (out.cpu().double() - want).abs()
            assert out.dtype == torch.float32 and bool((err <= bound).all()), (what, "reconstruct", mean is not None, scale,
                                                                                float((err / (bound + 1e-300)).max()))
        if c.r:
            six = dict(zip(bm.KEYS, OPS.recon_error(Uh, Ul, coef, mdev, orig).cpu().tolist()))
            diag_check(six, c.orig, Uh_c, Ul_c, c.c_high(), c.c_low(), what=(what, "recon_error", mean is not None), mean=mean)


@pytest.mark.parametrize("fp16", [True, False], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rows", [257, 4097])
def test_reconstruct_and_recon_error_against_fp64(rows, fp16):
    for k, nl in bm.PAIRS + [(0, 0)]:
        c = bm.Case(rows, k, nl, fp16)
        _check_ops(c, *_on(c), what=(rows, k, nl, fp16))


@pytest.mark.parametrize("rows", [257, 4097])
def test_mixed_basis_types_are_lifted_never_rounded(rows):
    """U_high fp16 beside a float32 U_low whose values fp16 cannot hold, and the reverse: the result is inside the bound of
    the tensors as given (the reference computes ``U_high.float() @ c_high + U_low.float() @ c_low``).  The element type
    used to be taken from U_high alone, which rounded a float32 U_low to fp16 -- an error of 2^-11 of every product,
    a thousand times the bound.  bf16 arrays are lifted exactly.  The Python wrappers of the same kernels follow the
    same rule."""
    import svdq_amd
    d = dev()
    for k, nl in [(2, 2), (1, 3), (7, 9), (0, 4), (4, 0)]:
        c = bm.Case(rows, k, nl, False)      # float32 values: not representable in fp16
        assert k == 0 or not torch.equal(c.U_high.half().float(), c.U_high)
        for high, low in ((torch.float16, None), (None, torch.float16), (torch.bfloat16, torch.bfloat16),
                          (torch.bfloat16, None), (torch.float16, torch.bfloat16)):
            Uh, Ul = _on(c, high, low)
            _check_ops(c, Uh, Ul, what=(rows, k, nl, high, low))
            if k + nl and torch.bfloat16 not in (high, low):
                x = c.orig.to(d)
                six = svdq_amd.diagnostics._fused_error(x, Uh, Ul, c.c_high().to(d), c.c_low().to(d), d)
                diag_check(six, c.orig, Uh.cpu(), Ul.cpu(), c.c_high(), c.c_low(), what=("_fused_error", rows, k, nl, high, low))
                out = svdq_amd.merge._reconstruct(c.c_high().to(d), c.c_low().to(d), Uh, Ul, c.mean.to(d), 0.5)
                want, bound = bm.reconstruct_exact(Uh.cpu(), Ul.cpu(), c.coef, c.mean, 0.5)
                assert bool(((out.cpu().double() - want).abs() <= bound).all()), ("_reconstruct", rows, k, nl, high, low)
                ch, cl = svdq_amd.compress._project(c.delta.to(d), Uh, Ul, c.mean.to(d))
                want, bound = bm.project_exact(Uh.cpu(), Ul.cpu(), c.delta, c.mean)
                got = torch.cat([ch, cl]).cpu().double()
                assert bool(((got - want).abs() <= bound).all()), ("_project", rows, k, nl, high, low)


def test_reconstruct_and_recon_error_refusals():
    d = dev()
    c = bm.Case(257, 2, 2, True)
    Uh, Ul = _on(c)
    coef, mean, orig = c.coef.to(d), c.mean.to(d), c.orig.to(d)
    wide = torch.zeros(257, 31, dtype=torch.float16, device=d)
    for bad, fragment in [
        (lambda: OPS.reconstruct(Uh[:, 0], Ul, coef, mean, 1.0), r"U_high \[D, k\] and U_low \[D, n_low\]"),
        (lambda: OPS.reconstruct(Uh[:200], Ul, coef, mean, 1.0), r"U_high \[D, k\] and U_low \[D, n_low\]"),
        (lambda: OPS.reconstruct(wide, Ul, torch.zeros(33, device=d), mean, 1.0), "at most 32 basis columns"),
        (lambda: OPS.reconstruct(Uh, Ul, coef[:3], mean, 1.0), "Shape mismatch: 3 coefficients for 4 basis columns"),
        (lambda: OPS.reconstruct(Uh, Ul, coef, mean[:200], 1.0), "mean has 200 elements"),
        (lambda: OPS.recon_error(Uh, Ul, coef, mean[:200], orig), "mean has 200 elements"),
        (lambda: OPS.recon_error(Uh, Ul, coef, None, orig[:200]), "Shape mismatch: original has 200 elements"),
        (lambda: OPS.recon_error(Uh, Ul, coef[:3], None, orig), "Shape mismatch: 3 coefficients"),
    ]:
        with pytest.raises(ValueError, match=fragment):
            bad()
    # a mean of shape [D, 1], a CPU coefficient vector and a float64 orig are taken as their values
    out = OPS.reconstruct(Uh, Ul, c.coef, mean.view(-1, 1), 0.5)
    assert torch.equal(out, OPS.reconstruct(Uh, Ul, coef, mean, 0.5))
    assert torch.equal(OPS.recon_error(Uh, Ul, c.coef, None, orig.double()), OPS.recon_error(Uh, Ul, coef, None, orig))
