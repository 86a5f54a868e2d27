"""
The row identities of tests/test_hip_basis_rows.py (helpers.basis_rows_check) on the REFERENCE chain, without a GPU:
LAPACK fp32 SVD, the ``.half()`` cast and fp32 GEMVs -- what the kernels replace -- must satisfy the bounds with the
committed constants (which were fitted on this chain over the GPU module's whole shape list, as twice what it needs),
and four faults of the kind a streaming kernel can have, planted in the reference's output, must each exceed them at
least twentyfold.  The shape list is a reduced one so that the module stays under a minute.
"""
import numpy as np
import pytest
import torch

from helpers import basis_rows_inputs, basis_rows_ratios, basis_rows_check, reference_chain

SHAPES = [(1, 1), (2, 2), (7, 8), (255, 4), (257, 16), (4099, 8), (8193, 32), (20000, 17), (70001, 20), (300001, 8)]
FAULT_SHAPES = [(4099, 8), (20000, 17), (70001, 20)]


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle
    return svd_hybrid_oracle


@pytest.mark.parametrize("D,N", SHAPES)
def test_reference_chain_satisfies_row_identities(orc, D, N):
    deltas = basis_rows_inputs(orc, D, N)
    for center in (True, False):
        for fp16 in (True, False):
            U_high, U_low, mean, coef, sigma = reference_chain(orc, deltas, center, fp16)
            what = f"reference D={D} N={N} center={center} fp16={fp16}"
            s = basis_rows_check(deltas, U_high, U_low, mean, coef, sigma, fp16, center, what=what)
            print(f"basis_rows {what} a={s['a']:.3f} a0={s['a0']:.3f} g_need={s['a_need']:.3f} b={s['b']:.3f} c={s['c']:.3f} "
                  f"c_need={s['c_need']:.2f} c_err={s['c_err']:.2e}")
            # no direction of these inputs sits in the band the library documents as poorly resolved (< 1e-5 sigma_0),
            # apart from the one exact null direction of a centred stack: nothing had to be left out of (c)
            if D > N:
                S = s["S64"][:-1] if center else s["S64"]
                assert S.size == 0 or S.min() > 1e-5 * s["S64"][0], (what, s["S64"])


def _faults(U, mean, D, row):
    """(name, U', mean') for each planted fault; ``row`` is a row of typical size away from the spikes."""
    out = []
    V = U.clone()
    V[row] = 0
    out.append(("one row of U zeroed", V, mean))
    V = U.clone()
    V[[row, row + 1]] = U[[row + 1, row]]
    out.append(("two adjacent rows of U swapped", V, mean))
    b = (row // 256) * 256
    e = min(b + 256, D)
    V = U.clone()
    V[b + 1:e] = U[b:e - 1]
    out.append(("one 256-row block of U shifted by one row", V, mean))
    if mean is not None:
        m = mean.clone()
        m[D - D % 256:] = 0
        out.append(("the last D mod 256 rows of the mean zeroed", U, m))
    return out


@pytest.mark.parametrize("D,N", FAULT_SHAPES)
def test_checker_catches_planted_faults(orc, D, N):
    assert D % 256 != 0
    deltas = basis_rows_inputs(orc, D, N)
    T = torch.stack(deltas, dim=1).double()
    for center in (True, False):
        size = (T - T.mean(dim=1, keepdim=True) if center else T).abs().amax(dim=1)
        size[-1] = float("inf")                        # (the swap needs a row below it)
        row = int(size.argsort()[D // 2])              # the median row: neither a spike nor a row that happens to be ~0
        for fp16 in (True, False):
            U_high, U_low, mean, coef, sigma = reference_chain(orc, deltas, center, fp16)
            k = U_high.shape[1]
            U = torch.cat([U_high, U_low], dim=1)
            for name, V, m in _faults(U, mean, D, row):
                what = f"{name}: D={D} N={N} center={center} fp16={fp16}"
                s = basis_rows_ratios(deltas, V[:, :k], V[:, k:], m, coef, sigma, fp16, center)
                worst = max(s["a"], s["b"], s["c"])
                print(f"basis_rows fault {what} a={s['a']:.1f} b={s['b']:.1f} c={s['c']:.1f}")
                assert worst >= 20.0, (what, s["a"], s["b"], s["c"])
                if D == FAULT_SHAPES[0][0]:
                    with pytest.raises(AssertionError):
                        basis_rows_check(deltas, V[:, :k], V[:, k:], m, coef, sigma, fp16, center, what=what)
