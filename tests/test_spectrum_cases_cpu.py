"""
The eigen-stage sweep of tests/test_hip_spectrum_sweep.py without a GPU: a numpy model of what the kernels compute --
fp32 row mean and fp32 centring, fp64 Gram of the fp32 values, the ``C G C`` deflation of 1 / sqrt(N), ``eigvalsh``, the
fp32 rank rule -- goes through the same checker (spectrum_cases.check_spectrum) on the same inputs for every (kind, N),
and must stay at or below a TENTH of every bound: the inputs and the fp64 truth leave the device that much room.  Four
faults of the kind the eigen stage can have, planted in the model, must each exceed the bounds at N = 8, 20 and 32.

Worst error / bound of the model per kind over N = 1 .. 32 (every picked threshold, 0.9 where the rank is decidable,
1.0 with max_rank 1 and 3); tests/test_hip_spectrum_sweep.py has the table by part, beside the device's:
  graded 0.015   graded_c 0.031   gap 0.012   gap_c 0.021   dependent 0.012   twins_c 0.018   short 0.012   short_c 0.012
  band 0.018   band_c 0.012
Planted faults at N = 8 / 20 / 32: fp32 products 414 / 1160 / 782 (graded), 117 / 155 / 64 (gap); no deflation 1.5 / 3.8 /
5.5 (graded_c: the residue of the fp32 centring along 1 / sqrt(N), reported where the truth has a zero); last task
dropped from the Gram 5e4 (graded: the smallest sigma lost) and infinite (gap_c: k moves).
"""
import numpy as np
import pytest
import torch

import spectrum_cases as sc

MODEL_MAX = 0.1
FAULT_N = [8, 20, 32]


def cum_f32(sig):
    S = np.asarray(sig, dtype=np.float32)
    total = np.float32(0)
    for x in S:
        total = np.float32(total + x * x)
    cum = np.ones(S.size, dtype=np.float32)
    if not total < np.float32(1e-10):
        run = np.float32(0)
        for i, x in enumerate(S):
            run = np.float32(run + x * x)
            cum[i] = run / total
    return cum


def rank_rule(sig, thr, max_rank, thr_fp64=False):
    """svdq_eig.h: fp32 squares summed in order, cum = run / total, k = #(cum < thr) + 1 with the threshold compared as
    fp32, then the clamps.  ``thr_fp64``: the planted fault -- the comparison done in fp64.  Returns (k, energy)."""
    cum = cum_f32(sig)
    r = cum.size
    t = float(thr) if thr_fp64 else np.float32(thr)
    k = 1 + int(sum((float(c) < t) if thr_fp64 else (c < t) for c in cum))
    if max_rank:
        k = min(k, max_rank)
    k = min(k, r)
    return k, (float(cum[k - 1]) if k > 0 else 0.0)


def model_sigma(deltas, center, fault=None):
    T = torch.stack([d.reshape(-1) for d in deltas], dim=1).numpy()      # [D, N] fp32
    D, N = T.shape
    if center:
        s = np.zeros(D, dtype=np.float32)
        for t in range(N):      # task order, one divide, like the streaming kernels
            s = s + T[:, t]
        T = T - (s / np.float32(N))[:, None]
    if fault == "fp32 products":
        G = np.zeros((N, N))
        for lo in range(0, D, 1024):      # every product rounded to fp32, summed in fp64
            X = T[lo:lo + 1024]
            G += (X[:, :, None] * X[:, None, :]).astype(np.float64).sum(axis=0)
    else:
        X = T.astype(np.float64)
        G = X.T @ X
    if fault == "last task dropped from the Gram":
        G[-1, :] = 0.0
        G[:, -1] = 0.0
    if center and fault != "no deflation":
        C = np.eye(N) - np.full((N, N), 1.0 / N)
        G = C @ G @ C
    lam = np.linalg.eigvalsh(0.5 * (G + G.T))[::-1]
    return np.sqrt(np.clip(lam, 0.0, None))[:min(D, N)].astype(np.float32)


def settings_of(S64):
    out = [(thr, None) for thr, _ in sc.pick_thresholds(S64)]
    if sc.rank_decidable(S64, 0.9, None):
        out.append((0.9, None))
    return out or [(2.0, None)]      # nothing decidable: every cumulative energy is below 2, k = r


@pytest.mark.parametrize("N", sc.N_ALL)
def test_model_within_a_tenth_of_every_bound(N):
    for center in (False, True):
        for name, kind, D in sc.cases_of(N, center):
            deltas = sc.make_case(kind, N, D)
            S64 = sc.truth_sigma(deltas, center)
            assert S64.size == min(D, N)
            sig = model_sigma(deltas, center)
            worst, parts = 0.0, {}
            for thr, mr in settings_of(S64) + [(1.0, 1), (1.0, 3)]:
                if not sc.rank_decidable(S64, thr, mr):
                    continue
                k, en = rank_rule(sig, thr, mr)
                d = {}
                w = sc.check_spectrum(sig, k, en, S64, thr, mr, center, detail=d)
                if w >= worst:
                    worst, parts = w, d
            print(f"spectrum model N={N} center={center} {name}: worst {worst:.4f} {parts}")
            assert worst <= MODEL_MAX, (N, center, name, worst, parts)


def test_thresholds_exist_for_every_task_count():
    """The rank rule is exercised at every N >= 3: ``graded`` or ``gap`` offers at least one threshold in a gap of 2e-4
    between cumulative energies (``graded`` from N = 8 on; ``gap``, whose tail decays gently, below)."""
    for N in sc.N_ALL:
        if N < 3:
            continue
        got = {kind: sc.pick_thresholds(sc.truth_sigma(sc.make_case(kind, N), False)) for kind in ("graded", "gap")}
        print(f"spectrum thresholds N={N}: " + "  ".join(f"{k_} k={[k for _, k in v]}" for k_, v in got.items()))
        assert got["graded"] or got["gap"], N
        if N >= 8:
            assert got["graded"], N
        for v in got.values():
            for thr, _ in v:
                assert float(np.float32(thr)) == thr and 0.0 < thr < 1.0


@pytest.mark.parametrize("N", FAULT_N)
def test_checker_catches_planted_faults(N):
    def ratio(kind, center, fault):
        deltas = sc.make_case(kind, N)
        S64 = sc.truth_sigma(deltas, center)
        sig = model_sigma(deltas, center, fault)
        worst = 0.0
        for thr, mr in settings_of(S64):
            k, en = rank_rule(sig, thr, mr)
            worst = max(worst, sc.check_spectrum(sig, k, en, S64, thr, mr, center))
        return worst

    for kind, center, fault in (("graded", False, "fp32 products"), ("gap", False, "fp32 products"),
                                ("graded_c", True, "no deflation"),
                                ("graded", False, "last task dropped from the Gram"),
                                ("gap_c", True, "last task dropped from the Gram")):
        good, bad = ratio(kind, center, None), ratio(kind, center, fault)
        print(f"spectrum fault N={N} {kind}: {fault}: {bad:.3g} (sound model {good:.4f})")
        assert good <= MODEL_MAX and bad > 1.0, (N, kind, fault, good, bad)
    # The rank rule with the threshold compared in fp64: a threshold a quarter ulp above a cumulative energy -- a margin
    # below 1e-7, on purpose -- rounds to that energy in fp32, where `cum < thr` is false; in fp64 it is true and k grows by one.
    # Fed with the truth itself, so nothing but the comparison differs.
    # The case: a cumulative energy that the rule's in-order fp32 sums and the truth's (torch's) agree on to the bit.
    for kind in ("graded", "gap"):
        S64 = sc.truth_sigma(sc.make_case(kind, N), False)
        S32 = S64.astype(np.float32)
        cum, own = sc.truth_rank_energy(S64, 0.5, None)[2], cum_f32(S32)
        js = [j for j in range(S32.size - 1) if own[j] == cum[j] and cum[j + 1] - cum[j] > 1e-5]
        if js:
            break
    j = js[0]
    thr = float(cum[j]) + 0.25 * float(np.spacing(cum[j]))      # a quarter of an fp32 ulp: 1.5e-8 at the most
    assert float(np.float32(thr)) == float(cum[j]) and thr > float(cum[j])
    k, en = rank_rule(S32, thr, None)
    assert sc.check_spectrum(S32, k, en, S64, thr, None, False) <= MODEL_MAX
    kf, enf = rank_rule(S32, thr, None, thr_fp64=True)
    assert kf == k + 1
    assert sc.check_spectrum(S32, kf, enf, S64, thr, None, False) == float("inf")
