"""
The register form of pass 1 (csrc/svdq_gram.hip, 1 <= N <= 8) against its numpy model, BIT FOR BIT (run with ``-m gpu``
on an MI355X).

What is compared is the reduced Gram that pass 1 + k_reduce leave in the plan's workspace (SVDQ_RC chunks of N x N
doubles per parameter) with tests/gram_registers_model.py, which repeats the kernel's sums in the kernel's order; the
model itself is held to the forward-error bound of an fp64 sum by tests/test_gram_registers_cpu.py.  Then sigma, k, r
and the energy of the following eigen stage against fp64 truth and the oracle's rank rule, with the bounds and the
"rank decidable" convention of the spectrum sweep (tests/spectrum_cases.py).

Task counts 1, 3, 4, 5, 7, 8 (both kernels, FULL and padded); per plan the row counts 1, 3 (a partial first f32x4), 255,
256, 257 (the block edge), 4095, 4097 (the unit edge at 4096-row units) and 8193 (three units, a ragged tail) as eight
parameters, so that every parameter's first unit follows another one's tail; centre on and off; fp16 / bf16 inputs;
minus-base; one gather and one walk plan whose masks leave a partial last block.  Inputs: the oracle's synthetic deltas
plus one task-dependent spike per 256-row block (gram_registers_model.spiked_deltas).
"""
import functools

import numpy as np
import pytest
import torch

import gram_registers_model as gm
import spectrum_cases as sc

pytestmark = pytest.mark.gpu
TASKS = [1, 3, 4, 5, 7, 8]
ROWS = [1, 3, 255, 256, 257, 4095, 4097, 8193]
UNIT_ROWS = 4096
THR = 0.9
KW = dict(energy_threshold=THR, max_rank=None, fp16=True, low_bits=4, rtvq_stages=2)


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _deltas(D, N, seed):
    """N fp32 numpy arrays; computed once, shared, never written to."""
    from oracle import svd_hybrid_oracle as orc
    out = gm.spiked_deltas([d.numpy() for d in orc.synthetic_deltas(D, N, seed, rank=min(3, N))])
    for d in out:
        d.setflags(write=False)
    return tuple(out)


def _to_dev(arrays, dtype=torch.float32):
    return [torch.from_numpy(np.array(a)).to(_dev()).to(dtype).contiguous() for a in arrays]


def _table(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(_dev())


def _gram2(plan):
    """[P, RC, N, N] fp64: the level-2 Gram partials in the plan's workspace."""
    P, N = plan.P, plan.N
    off = gm.workspace_gram2_offset(int(plan.sizes.n_slots), P, N)
    nbytes = P * gm.RC * N * N * 8
    torch.cuda.synchronize()
    return plan.workspace[off:off + nbytes].view(torch.float64).cpu().numpy().reshape(P, gm.RC, N, N)


def _check_gram(plan, rows_per_param, unit_rows, what):
    """``rows_per_param``: the centred fp32 rows [D, N] of every parameter as the route under test sees them."""
    got = _gram2(plan)
    for p, xc in enumerate(rows_per_param):
        want = gm.gram_chunks(xc, unit_rows, plan.rows[p])
        same = got[p].view(np.uint64) == want.view(np.uint64)
        if not same.all():
            c, i, j = [int(x[0]) for x in np.nonzero(~same)]
            raise AssertionError(f"{what} parameter {p} ({xc.shape[0]} rows): {int((~same).sum())} of {same.size} "
                                 f"doubles differ, first at chunk {c} entry ({i}, {j}): {got[p, c, i, j]!r} against "
                                 f"the model's {want[c, i, j]!r}")


def _check_eig(plan, deltas_per_param, center, what):
    sm = plan.fetch_small()
    N = plan.N
    for p, deltas in enumerate(deltas_per_param):
        D = deltas[0].shape[0]
        S64 = sc.truth_sigma([torch.from_numpy(np.array(d)) for d in deltas], center)
        r = int(sm.r[p])
        assert r == min(D, N) and int(sm.rows[p]) == D, (what, p, r, int(sm.rows[p]))
        k, en = int(sm.k[p]), float(sm.energy[p])
        if not sc.rank_decidable(S64, THR, None):
            k, en, _ = sc.truth_rank_energy(S64, THR, None)
        parts = {}
        w = sc.check_spectrum(sm.sigma[p, :r], k, en, S64, THR, None, center, detail=parts)
        print(f"gram registers {what} parameter {p} D={D}: spectrum error / bound {w:.4f} {parts}")
        assert w <= 1.0, (what, p, D, w, parts, sm.sigma[p, :r], S64)


def _plain_plan(sq, N, rows, center, seeds, dtype=torch.float32):
    from svdq_amd.pipeline import CompressPlan
    deltas = [_deltas(D, N, s) for D, s in zip(rows, seeds)]
    if dtype is not torch.float32:      # the values the kernel reads: rounded to the input type once, exact from there on
        deltas = [tuple(torch.from_numpy(np.array(d)).to(dtype).float().numpy() for d in ds) for ds in deltas]
    plan = CompressPlan(rows, N, center=center, device=_dev(), unit_rows=UNIT_ROWS, input_dtype=dtype, **KW)
    vecs = [_to_dev(ds, dtype) for ds in deltas]
    tab = plan.pointer_table(vecs)
    plan.gram_center(tab)
    plan.eig_rank_select(tab)
    return plan, deltas


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("N", TASKS)
def test_plain_every_row_count(sq, N, center):
    plan, deltas = _plain_plan(sq, N, ROWS, center, [900 + i for i in range(len(ROWS))])
    what = f"plain N={N} center={center}"
    _check_gram(plan, [gm.centre(ds, center) for ds in deltas], UNIT_ROWS, what)
    _check_eig(plan, deltas, center, what)
    plan.close()


@pytest.mark.parametrize("N,center", [(8, True), (5, False)])
def test_two_parameter_plan(sq, N, center):
    """A unit of parameter 1 follows parameter 0's one-row tail unit."""
    plan, deltas = _plain_plan(sq, N, [4097, 257], center, [921, 922])
    what = f"two parameters N={N} center={center}"
    _check_gram(plan, [gm.centre(ds, center) for ds in deltas], UNIT_ROWS, what)
    _check_eig(plan, deltas, center, what)
    plan.close()


@pytest.mark.parametrize("dtype,N", [(torch.float16, 8), (torch.bfloat16, 8), (torch.float16, 3), (torch.bfloat16, 5)])
def test_half_inputs(sq, dtype, N):
    rows = [3, 257, 4097]
    plan, deltas = _plain_plan(sq, N, rows, True, [931, 932, 933], dtype=dtype)
    what = f"{dtype} N={N}"
    _check_gram(plan, [gm.centre(ds, True) for ds in deltas], UNIT_ROWS, what)
    _check_eig(plan, deltas, True, what)
    plan.close()


@pytest.mark.parametrize("N,center", [(8, True), (4, False), (7, True)])
def test_minus_base(sq, N, center):
    """Fine-tuned tensors and a base: the difference is formed in registers, in fp32."""
    from svdq_amd.pipeline import CompressPlan
    rows = [3, 4097, 8193]
    base = [_deltas(D, 1, 940 + i)[0] for i, D in enumerate(rows)]
    ft = [[(d + b).astype(np.float32) for d in _deltas(D, N, 950 + i)] for i, (D, b) in enumerate(zip(rows, base))]
    plan = CompressPlan(rows, N, center=center, device=_dev(), unit_rows=UNIT_ROWS, **KW)
    ft_dev, base_dev = [_to_dev(f) for f in ft], _to_dev(base)
    plan.run_from_base(plan.pointer_table(ft_dev), _table(base_dev))
    what = f"minus-base N={N} center={center}"
    _check_gram(plan, [gm.centre(f, center, base=b) for f, b in zip(ft, base)], UNIT_ROWS, what)
    _check_eig(plan, [[f - b for f in fs] for fs, b in zip(ft, base)], center, what)
    plan.close()


def _masked_inputs(N, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    deltas = [_deltas(D, N, seed + 1 + i) for i, D in enumerate(sizes)]
    masks = [(torch.rand(D, generator=g) < 0.6) for D in sizes]
    for m in masks:
        assert int(m.sum()) % gm.BLK != 0           # a partial last block
    compacted = [[np.ascontiguousarray(d[m.numpy()]) for d in ds] for ds, m in zip(deltas, masks)]
    return deltas, masks, compacted


@pytest.mark.parametrize("N", [8, 3])
def test_gather(sq, N):
    from svdq_amd.pipeline import CompressPlan
    from svdq_amd.mask_loader import MaskSet
    sizes = [3001, 700]
    deltas, masks, compacted = _masked_inputs(N, sizes, 960)
    masks_dev = [m.to(_dev()) for m in masks]
    ms = MaskSet(sizes, _dev())
    it, _, ct, _ = ms.indices(masks_dev, want_false=True)
    plan = CompressPlan(sizes, N, center=True, device=_dev(), unit_rows=1024, **KW)
    vecs = [_to_dev(ds) for ds in deltas]
    plan.run_gather(plan.pointer_table(vecs), _table(it), ct)
    what = f"gather N={N}"
    _check_gram(plan, [gm.centre(c, True) for c in compacted], 1024, what)
    _check_eig(plan, compacted, True, what)
    plan.close()


@pytest.mark.parametrize("N", [8, 3])
def test_walk(sq, N):
    from svdq_amd.pipeline import CompressPlan
    from svdq_amd.mask_loader import MaskSet
    sizes = [3001, 700]
    deltas, masks, compacted = _masked_inputs(N, sizes, 970)
    masks_dev = [m.to(_dev()) for m in masks]
    ms = MaskSet(sizes, _dev())
    ct, _ = ms.count_scan(masks_dev)
    mtab = _table(ms._s["mb"])
    plan = CompressPlan(sizes, N, center=True, device=_dev(), unit_rows=1024, **KW)
    us = ms.unit_starts(plan, ct)
    vecs = [_to_dev(ds) for ds in deltas]
    plan.run_masked(plan.pointer_table(vecs), mtab, us, ct)
    what = f"walk N={N}"
    _check_gram(plan, [gm.centre(c, True) for c in compacted], 1024, what)
    _check_eig(plan, compacted, True, what)
    plan.close()
