"""Inputs, fp64 truth and the checker of the eigen-stage sweep (tests/test_spectrum_cases_cpu.py on a numpy model of the
kernel, tests/test_hip_spectrum_sweep.py on the device).  numpy / torch on the CPU only; nothing is read from disk.

Inputs   ``T = Q diag(sigmas) Z^T`` with orthonormal Q [D, m] and Z [N, m], built in fp64 and cast to fp32 -- the method
         of the graded golden chains (tests/golden/make_golden.py, ``_structured`` / ``_structured_centred``), restated.
         Centred kinds take the columns of Z orthogonal to the ones vector and add a common per-row offset
         ``cm * randn(D, 1)``, which is what centring removes.  D = 6007: two 4096-row units with a ragged tail.  The seed
         is a fixed function of (kind, N).

  kind        N     sigmas / sigma_0                                                               centred
  graded      >= 1  10 ** (-4.5 i / max(N - 1, 1)), i = 0 .. N-1 (down to 3.2e-5)                  no
  graded_c    >= 2  the same law over N - 1 values, cm = 0.3                                       yes
  gap         >= 3  10 ** (-1.5 i / (N - 2)) for N - 1 values, then one at 1e-4                    no
  gap_c       >= 3  the same law over N - 2 values, then 1.3e-4, cm = 0.2                          yes
  dependent   >= 3  the first N - 1 tasks of ``gap``, last task = task 0 + task 1 (the fp32 sum)   no
  twins_c     >= 3  ``gap_c`` of N - 1 tasks, task 1 repeated as the last task                     yes
  band        >= 2  10 ** (-2.6 i / (N - 1)), i = 0 .. N-1 (down to 2.5e-3, nothing below)         no
  band_c      >= 2  the same law over N - 1 values, cm = 0.3                                       yes
  short       >= 2  N - 1 and N rows, singular values spread evenly over [0.2, 1]                  no
  short_c     >= 2  the same with cm = 0.3                                                         yes

         ``gap`` / ``gap_c`` end in lambda = 1e-8 lambda_0, below what sums of fp32 products resolve: above 16 tasks
         the surplus-null trigger of the eigen stage has to ask for the exact-product pass.  ``short`` has D < N (r = D).
         ``band`` / ``band_c`` (an addition to the kinds the sweep was specified with) end a decade under the 2e-2 sigma_0
         edge of the refinement band with nothing lower, so that above 16 tasks only that edge asks for the pass: sums
         of fp32 products are off by a few 1e-9 lambda_0 (measured: tests/test_hip_spectrum_sweep.py), i.e. by
         ~3e-4 of a sigma at 2.5e-3 sigma_0, fifteen times the bound.

Truth    ``numpy.linalg.svd`` in fp64 of the fp32 stack, centred EXACTLY in fp64 when the plan is centred: it has an
         exact zero where the kernel deflates 1 / sqrt(N), so no residue has to be taken out of the list.  Rank and
         retained energy: the reference's fp32 rule (oracle.select_rank / energy_spectrum) on those values cast to fp32.

Checker  ``check_spectrum``; every figure is that of test_hip_parity.test_small_singular_values_vs_reference_vectors.
"""
import numpy as np
import torch

D_SWEEP = 6007
N_ALL = list(range(1, 33))
KINDS = ("graded", "graded_c", "gap", "gap_c", "dependent", "twins_c", "short", "short_c", "band", "band_c")
CENTRED = {"graded": False, "graded_c": True, "gap": False, "gap_c": True, "dependent": False, "twins_c": True,
           "short": False, "short_c": True, "band": False, "band_c": True}
MIN_N = {"graded": 1, "graded_c": 2, "gap": 3, "gap_c": 3, "dependent": 3, "twins_c": 3, "short": 2, "short_c": 2,
         "band": 2, "band_c": 2}

SIGMA_RTOL = 2e-5        # resolved directions, relative to the fp64 value
CENTRED_FLOOR = 1e-9     # ... plus this much of sigma_0 on a centred plan: one ulp of the fp32 row mean moves a small
#                          sigma by ~(ulp noise)^2 / 2 sigma (the comment in the test the figures come from)
RESOLVED = 1e-6          # sigma64 > RESOLVED sigma64_0: a direction the fp32 data resolves
NULL_BOUND = 2e-6        # what is reported for an unresolved one, in sigma_0
ENERGY_ATOL = 2e-5       # the seeded tests' figure; follows from 2e-5 on sigma: 4 * 2e-5 * cum (1 - cum) <= 2e-5
THR_GAP = 2e-4           # a threshold sits in the middle of a gap of at least this much between cumulative energies


def seed_of(kind, N, extra=0):
    return 100003 * (KINDS.index(kind) + 1) + 101 * N + extra


def _orthonormal(rng, rows, cols):
    Q, _ = np.linalg.qr(rng.standard_normal((rows, cols)))
    return Q


def _to_tasks(T):
    return [torch.from_numpy(np.ascontiguousarray(T[:, j]).astype(np.float32)) for j in range(T.shape[1])]


def structured(D, N, sigmas, seed):
    """T = Q diag(sigmas) Z^T, m = len(sigmas) <= min(D, N) columns in Q [D, m] and Z [N, m]; N fp32 tensors."""
    rng = np.random.default_rng(seed)
    m = len(sigmas)
    Q = _orthonormal(rng, D, m)
    Z = _orthonormal(rng, N, N)[:, :m]
    return _to_tasks((Q * np.asarray(sigmas, dtype=np.float64)) @ Z.T)


def structured_centred(D, N, sigmas, seed, cm):
    """T = Q diag(sigmas) Z^T + c 1^T with the m <= N - 1 columns of Z orthonormal and orthogonal to the ones vector:
    the centred stack has the singular values given, and the common offset c = cm * randn(D, 1) is what centring removes."""
    rng = np.random.default_rng(seed)
    m = len(sigmas)
    Q = _orthonormal(rng, D, m)
    M = np.concatenate([np.ones((N, 1)), rng.standard_normal((N, N - 1))], axis=1)
    Z = np.linalg.qr(M)[0][:, 1:1 + m]
    return _to_tasks((Q * np.asarray(sigmas, dtype=np.float64)) @ Z.T + cm * rng.standard_normal((D, 1)))


def graded_sigmas(n):
    return [10.0 ** (-4.5 * i / max(n - 1, 1)) for i in range(n)]


def band_sigmas(n):
    return [10.0 ** (-2.6 * i / max(n - 1, 1)) for i in range(n)]


def gap_sigmas(n, last):
    """n - 1 values falling gently to 10 ** -1.5, then ``last``."""
    return [10.0 ** (-1.5 * i / max(n - 2, 1)) for i in range(n - 1)] + [last]


def _short_sigmas(m):
    return list(np.linspace(1.0, 0.2, m)) if m > 1 else [1.0]


def exists(kind, N):
    return N >= MIN_N[kind]


def make_case(kind, N, D=None):
    """The N task tensors (fp32, CPU) of one case; ``short`` kinds take D = N - 1 or N, the others D = 6007."""
    assert exists(kind, N), (kind, N)
    if kind in ("short", "short_c"):
        assert D in (N - 1, N), (kind, N, D)
        seed = seed_of(kind, N, D)
        if kind == "short":
            return structured(D, N, _short_sigmas(min(D, N)), seed)
        return structured_centred(D, N, _short_sigmas(min(D, N - 1)), seed, 0.3)
    D = D_SWEEP if D is None else D
    seed = seed_of(kind, N)
    if kind == "graded":
        return structured(D, N, graded_sigmas(N), seed)
    if kind == "graded_c":
        return structured_centred(D, N, graded_sigmas(N - 1), seed, 0.3)
    if kind == "band":
        return structured(D, N, band_sigmas(N), seed)
    if kind == "band_c":
        return structured_centred(D, N, band_sigmas(N - 1), seed, 0.3)
    if kind == "gap":
        return structured(D, N, gap_sigmas(N, 1e-4), seed)
    if kind == "gap_c":
        return structured_centred(D, N, gap_sigmas(N - 1, 1.3e-4), seed, 0.2)
    if kind == "dependent":
        ts = structured(D, N, gap_sigmas(N, 1e-4), seed)[:N - 1]
        return ts + [ts[0] + ts[1]]
    if kind == "twins_c":
        ts = structured_centred(D, N - 1, gap_sigmas(N - 2, 1.3e-4), seed, 0.2)
        return ts + [ts[1].clone()]
    raise ValueError(kind)


def cases_of(N, center):
    """[(name, kind, D)] of one plan: every kind of this centring that exists at N."""
    if N == 1 and center:      # no centred kind exists for one task: its centred stack is exactly zero, which is the case
        return [("graded", "graded", D_SWEEP)]
    out = []
    for kind in KINDS:
        if CENTRED[kind] != bool(center) or not exists(kind, N):
            continue
        if kind.startswith("short"):
            out += [(f"{kind}_d{D}", kind, D) for D in (N - 1, N)]
        else:
            out.append((kind, kind, D_SWEEP))
    return out


def truth_sigma(deltas, center):
    """fp64 singular values (min(D, N) of them) of the fp32 stack, centred exactly in fp64 when ``center``."""
    T = torch.stack([d.reshape(-1) for d in deltas], dim=1).double().numpy()
    if center:
        T = T - T.mean(axis=1, keepdims=True)
    return np.linalg.svd(T, compute_uv=False)


def truth_rank_energy(S64, thr, max_rank):
    """(k, retained energy, cumulative energies): the reference's fp32 rule on the fp64 values cast to fp32."""
    from oracle import svd_hybrid_oracle as orc
    S = torch.from_numpy(np.asarray(S64, dtype=np.float64)).float()
    k = orc.select_rank(S, thr, max_rank)
    cum = orc.energy_spectrum(S)
    return k, (float(cum[k - 1]) if k > 0 else 0.0), cum.numpy()


def rank_decidable(S64, thr, max_rank, margin=THR_GAP / 2):
    """True where no cumulative energy of the truth comes within ``margin`` of the threshold, or where the clamps decide
    the rank whichever side such a one falls on: the rank is then a property of the input, not of the last bit."""
    return truth_rank_energy(S64, thr - margin, max_rank)[0] == truth_rank_energy(S64, thr + margin, max_rank)[0]


def pick_thresholds(S64):
    """Up to three thresholds, each the fp32 midpoint between consecutive cumulative energies of the truth that lie at
    least THR_GAP apart -- from the start, the middle and the end of the usable range.  [(thr, k expected)]."""
    cum = truth_rank_energy(S64, 0.5, None)[2].astype(np.float64)
    usable = []
    for j in range(len(cum) - 1):
        if cum[j + 1] - cum[j] >= THR_GAP:
            thr = float(np.float32(0.5 * (cum[j] + cum[j + 1])))      # rounds to itself in fp32
            if min(thr - cum[j], cum[j + 1] - thr) >= 0.45 * THR_GAP:
                usable.append((thr, j + 2))
    if len(usable) <= 3:
        return usable
    return [usable[0], usable[len(usable) // 2], usable[-1]]


def check_spectrum(sigma, k, energy, truth, thr, max_rank, center, detail=None):
    """Worst error / bound ratio of one parameter's eigen-stage outputs against ``truth`` (fp64 singular values):
      resolved directions (S64 > 1e-6 s0)   |sigma - S64| <= 2e-5 S64 + floor, floor = 1e-9 s0 centred, 0 otherwise
      unresolved directions                  sigma <= 2e-6 s0
      k                                      equal to the truth's (a wrong rank is a ratio of infinity)
      energy                                 |energy - truth| <= 2e-5
    A NaN anywhere is a ratio of infinity.  ``detail``, when given, receives the parts."""
    S64 = np.asarray(truth, dtype=np.float64)
    sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
    inf = float("inf")
    if sg.shape != S64.shape:
        return inf
    r = S64.size
    s0 = float(S64[0]) if r else 0.0
    resolved = S64 > RESOLVED * s0
    floor = CENTRED_FLOOR * s0 if center else 0.0
    rs = rn = 0.0
    if resolved.any():
        rs = float(np.nan_to_num(np.abs(sg - S64)[resolved] / (SIGMA_RTOL * S64[resolved] + floor), nan=inf).max())
    if (~resolved).any():
        if s0 > 0:
            rn = float(np.nan_to_num(sg[~resolved] / (NULL_BOUND * s0), nan=inf).max())
        else:
            rn = 0.0 if np.all(sg == 0.0) else inf
    k_t, e_t, _ = truth_rank_energy(S64, thr, max_rank)
    rk = 0.0 if int(k) == k_t else inf
    re = abs(float(energy) - e_t) / ENERGY_ATOL
    if not np.isfinite(re):
        re = inf
    if detail is not None:
        detail.update({"sigma": rs, "null": rn, "k": (int(k), k_t), "energy": re})
    return max(rs, rn, rk, re)
