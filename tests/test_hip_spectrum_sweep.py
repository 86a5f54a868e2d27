"""
The eigen stage -- Gram (exact products up to 16 tasks; fp32 products, then the flagged exact-product pass, above),
deflation of 1 / sqrt(N), fp64 Jacobi, fp32 rank rule -- against fp64 truth at EVERY task count from 1 to 32, centred
and not (run with ``-m gpu`` on an MI355X).

The golden chains check small singular values at N = 6, 8, 16 and 20 only, and every other input of the suite above 16
tasks has its noise floor over the 2e-2 sigma_0 edge of the refinement band, so the flagged exact-product Gram kernels
at 24, 28 and 32 task slots, their masked reduce and second eigen launch did real work in no accuracy test.  Here every
N gets spectra that reach 3.2e-5 sigma_0 (``graded``), a lone direction at lambda = 1e-8 lambda_0 under a gentle tail
(``gap``), a tail that ends a decade under that edge with nothing lower (``band``), exactly dependent tasks, and fewer
rows than tasks; tests/spectrum_cases.py states inputs, truth and checker.

Per (N, centring) ONE plan holds every kind as a parameter; it is run once per chosen energy threshold (sigma must not
move by a bit, only the rank rule may), at threshold 1.0 and with max_rank 1 and 3.  On the first plan, per parameter:
sigma / k / energy (spectrum_cases.check_spectrum), column norms and orthonormality of the resolved directions (bounds of
test_small_singular_values_vs_reference_vectors), the coefficients as projections on the device's own basis
(helpers.own_projection_mismatch) and the in-pipeline quantizer bit for bit.  ``test_inputs_need_exact_products`` shows
that the same inputs MISS the sigma bound when the refinement is switched off, i.e. that the sweep depends on it.

Worst error / bound per kind over N = 1 .. 32 and every run of the plan (a wrong k would be infinite); the model is
that of tests/test_spectrum_cases_cpu.py, the device figures were measured after inputs, truth and bounds were fixed:
                                graded   graded_c  gap      gap_c    dependent  twins_c  short    short_c  band     band_c
  numpy model (CPU)   sigma     0.0051   0.0310    0.0029   0.0210   0.0026     0.0180   0.0029   0.0034   0.0028   0.0028
                      null      -        0.0036    -        0.0035   0.0000     0.0053   -        0.0114   -        0.0032
                      energy    0.0149   0.0119    0.0119   0.0089   0.0119     0.0149   0.0119   0.0119   0.0179   0.0119
  device (MI355X)     sigma     0.0051   0.0310    0.0029   0.0229   0.0026     0.0292   0.0146   0.0194   0.0028   0.0028
                      null      -        0.0031    -        0.0038   0.0090     0.0032   -        0.0041   -        0.0039
                      energy    0.0149   0.0119    0.0119   0.0119   0.0119     0.0149   0.0119   0.0119   0.0179   0.0179
  (0.003 on sigma is the fp32 rounding of the reported value; 0.0119 on the energy is four fp32 ulp between the in-order
  sums of the rule and torch's)
  fp32 products only (plan flag 2), error / bound of the smallest resolved sigma at N = 20, 24, 28, 32:
    graded 5e4 each (reported as 0)      gap 1.1e4, 490, 6.2e3, 7.1e3      band 10.9, 9.6, 28.8, 13.9
The module runs in about 7 s (82 tests, about 0.1 s each).
"""
import functools

import numpy as np
import pytest
import torch

import spectrum_cases as sc
from helpers import check_pipeline_quantizer, own_basis, own_projection_mismatch

pytestmark = pytest.mark.gpu
FP16_N = [3, 8, 13, 17, 20, 27, 32]
EXACT_N = [20, 24, 28, 32]
TWICE_N = (20, 32)
SETTINGS = dict(low_bits=4, rtvq_stages=2)


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle
    return svd_hybrid_oracle


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=4)
def _inputs(N, center):
    """[(name, D, host tensors, fp64 truth)] of one plan; computed once, shared by the tests of this (N, centring)."""
    out = []
    for name, kind, D in sc.cases_of(N, center):
        deltas = sc.make_case(kind, N, D)
        out.append((name, D, deltas, sc.truth_sigma(deltas, center)))
    return out


def _settings(cases):
    """(threshold, max_rank) of every run of the plan, the first one being the run that is checked in full."""
    thrs = []
    for _, _, _, S64 in cases:
        thrs += [t for t, _ in sc.pick_thresholds(S64) if t not in thrs]
    thrs = thrs or [0.9]
    return [(t, None) for t in thrs] + [(1.0, None), (thrs[0], 1), (thrs[0], 3)]


def _check_spectrum(sm, p, S64, D, N, thr, max_rank, center, what):
    """sigma always; k and energy where the truth's rank does not hang on a cumulative energy within 1e-4 of the
    threshold.  Prints the figure, then asserts.  Returns (ratio, rank was decidable)."""
    r = int(sm.r[p])
    assert r == min(D, N) and int(sm.rows[p]) == D, (what, r, int(sm.rows[p]))
    decidable = sc.rank_decidable(S64, thr, max_rank)
    k, en = int(sm.k[p]), float(sm.energy[p])
    if not decidable:
        k, en, _ = sc.truth_rank_energy(S64, thr, max_rank)
    parts = {}
    w = sc.check_spectrum(sm.sigma[p, :r], k, en, S64, thr, max_rank, center, detail=parts)
    print(f"spectrum sweep {what} thr={thr!r} max_rank={max_rank} decidable={decidable}: {w:.4f} {parts}")
    assert np.all(sm.sigma[p, r:] == 0.0), what
    assert w <= 1.0, (what, thr, max_rank, w, parts, sm.sigma[p, :r], S64)
    return w, decidable


def _check_basis(plan, sm, p, S64, D, what):
    """Unit norm and orthonormality of the resolved directions; past them a column is exactly zero or unit norm."""
    k, r = int(sm.k[p]), int(sm.r[p])
    U_high, U_low, _ = plan.basis_tensors(p, k, r, D)
    assert U_high.shape == (D, k) and U_low.shape == (D, r - k), what
    U = torch.cat([U_high, U_low], dim=1).double()
    norms = (U * U).sum(0).sqrt().cpu().numpy()
    s0 = float(S64[0])
    nres = int((S64 > sc.RESOLVED * s0).sum())
    assert np.all(np.abs(norms[:nres] - 1.0) < 2e-3 + 2e-7 * s0 / S64[:nres]), (what, norms)
    for j in range(nres, r):
        assert norms[j] == 0.0 or abs(norms[j] - 1.0) < 2e-3, (what, j, norms[j])
    gram = (U[:, :nres].T @ U[:, :nres]).cpu().numpy()
    smin = np.minimum.outer(S64[:nres], S64[:nres])
    err = np.abs(gram - np.eye(nres))
    assert np.all(err < 3e-3 + 2e-7 * s0 / smin), (what, float(err.max()) if nres else 0.0)


def _check_parameter(orc, plan, sm, p, deltas, S64, D, what):
    _check_basis(plan, sm, p, S64, D, what)
    k, r = int(sm.k[p]), int(sm.r[p])
    U, mu32 = own_basis(plan, p, k, r, D)
    for t in range(plan.N):
        m = own_projection_mismatch(U, mu32, deltas[t], sm.coef[p, t, :r], sm.sigma[p, :r], t)
        assert m is None, (what, m)
    if r - k >= 1:
        check_pipeline_quantizer(orc, plan, sm, p)


def _run(sq, vecs, center, fp16, thr, max_rank):
    return sq.compress_batch(vecs, energy_threshold=thr, max_rank=max_rank, center=center, fp16=fp16, device=_dev(),
                             **SETTINGS)


def _sweep(sq, orc, N, center, fp16, settings_limit=None):
    cases = _inputs(N, center)
    dev = _dev()
    vecs = [[d.to(dev) for d in deltas] for _, _, deltas, _ in cases]
    settings = _settings(cases)[:settings_limit]
    sigma0 = None
    decided = [0] * len(settings)
    for i, (thr, max_rank) in enumerate(settings):
        plan, sm = _run(sq, vecs, center, fp16, thr, max_rank)
        if i == 0:
            sigma0 = sm.sigma.copy()
            if N in TWICE_N:      # deterministic reductions: the same plan again, the small buffer byte for byte
                again, _ = _run(sq, vecs, center, fp16, thr, max_rank)
                assert np.array_equal(plan.small.cpu().numpy(), again.small.cpu().numpy()), (N, center, fp16)
                again.close()
        else:      # only the rank rule may move with the threshold
            assert np.array_equal(sm.sigma.view(np.uint32), sigma0.view(np.uint32)), (N, center, thr, max_rank)
        for p, (name, D, deltas, S64) in enumerate(cases):
            what = f"N={N} center={center} fp16={fp16} {name}"
            _, dec = _check_spectrum(sm, p, S64, D, N, thr, max_rank, center, what)
            decided[i] += int(dec)
            if i == 0:
                _check_parameter(orc, plan, sm, p, deltas, S64, D, what)
        plan.close()
    assert all(n > 0 for n in decided), (settings, decided)      # every run decided the rank of some parameter


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("N", sc.N_ALL)
def test_spectrum_every_task_count(sq, orc, N, center):
    _sweep(sq, orc, N, center, fp16=False)


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("N", FP16_N)
def test_spectrum_fp16_basis(sq, orc, N, center):
    """The same plan with the basis stored in fp16, at the first threshold."""
    _sweep(sq, orc, N, center, fp16=True, settings_limit=1)


@pytest.mark.parametrize("N", EXACT_N)
def test_inputs_need_exact_products(sq, N):
    """Plan flag 2 (SVDQ_SW_GRAM_F32: fp32 products at every N, no refinement pass): the smallest resolved sigma of
    ``graded``, of ``gap`` and of ``band`` must MISS the bound the sweep holds the default path to -- otherwise the sweep
    above would pass whether or not the flagged exact-product pass above 16 tasks did its work."""
    from svdq_amd.pipeline import CompressPlan
    dev = _dev()
    cases = [c for c in _inputs(N, False) if c[0] in ("graded", "gap", "band")]
    assert len(cases) == 3
    vecs = [[d.to(dev) for d in deltas] for _, _, deltas, _ in cases]
    plan = CompressPlan([D for _, D, _, _ in cases], N, energy_threshold=0.9, max_rank=None, center=False, fp16=False,
                        device=dev, flags=2, **SETTINGS)
    plan.run(plan.pointer_table(vecs))
    torch.cuda.synchronize()
    sm = plan.fetch_small()
    for p, (name, D, _, S64) in enumerate(cases):
        j = int((S64 > sc.RESOLVED * S64[0]).sum()) - 1
        err = abs(float(sm.sigma[p, j]) - S64[j])
        ratio = err / (sc.SIGMA_RTOL * S64[j])
        print(f"spectrum sweep fp32 products N={N} {name}: sigma_{j} = {sm.sigma[p, j]:.6e} vs {S64[j]:.6e}, "
              f"error / bound {ratio:.3g}")
        assert ratio > 1.0, (N, name, j, float(sm.sigma[p, j]), S64[j], ratio)
    plan.close()
