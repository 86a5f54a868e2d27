"""
fp64 model of the three caller-basis operators of csrc/svdq_basis_ops.hip -- ``svdq_project``, ``svdq_reconstruct`` and
``svdq_recon_error`` -- on the values AS STORED: an fp16 basis widens to fp64 exactly; coefficients, mean, delta and
orig are the fp32 numbers given.  Nothing here imports the library: the launch geometry is restated below, and the
bounds are derived from it, not fitted to what the kernels return.

Geometry (restated from the kernels; ``project_grid`` is not imported).  256 threads per block, ``grid =
clamp(ceil(rows / 2048), 1, 1024)`` blocks, thread ``g = block * 256 + tid`` visits rows ``g, g + grid * 256, ...``: at
most ``m = ceil(rows / (grid * 256))`` rows.  So a thread gets a second row above 256 rows, a second block starts above
2048, and a ninth row above 1024 * 2048.

Bounds, with u = 2^-24 (fp32 unit roundoff) and u64 = 2^-53.

``project``:  c_i = sum_d U_di x_d,  x_d = delta_d - mean_d.
  A thread forms x_d with one fp32 subtraction, x^_d = x_d (1 + d0), |d0| <= u, and runs ONE chain of at most m fmas
  per column: every product that enters the chain is then rounded at most m times (once by its own fma, once by each
  later one), so the thread's partial is  sum_d U_di x_d (1 + t_d)  with  |t_d| <= (1 + u)^(m + 1) - 1 <= (m + 2) u'
  and  u' = u / (1 - (m + 2) u)   [Higham, Accuracy and Stability, lemma 3.1; the +2 holds the subtraction and leaves
  one rounding spare].  The same holds for any other order of a thread's m products and m - 1 additions without fma
  (a product is rounded once, a sum of m terms at most m - 1 times more, pairwise fewer), which is why the CPU test can
  hold the bound against three legitimate evaluations.
  The thread partials (|partial| summing to at most (1 + (m + 2) u') A_i, A_i = sum_d |U_di| |x_d|) are widened to fp64
  exactly and added in fp64: 8 levels of the block tree and a serial sum over the grid, at most T = 8 + grid additions on
  any path, error <= T u64 / (1 - T u64) times the sum of their magnitudes.  One cast to fp32 ends it: u |c^_i|.
      |c^_i - c_i| <= E_i + u (|c_i| + E_i),   E_i = ((m + 2) u' + g64 (1 + (m + 2) u')) A_i,  g64 = T u64 / (1 - T u64)
  The fp64 term is ~1e-13 A_i at the largest grid -- negligible, but it is in the bound.

``reconstruct``:  out_d = ((sum_i U_di c_i) + mean_d) * scale.
  The r = k + nl products are summed in two fma chains joined by one addition: each product is rounded at most r + 1
  times whatever the order (``helpers.diag_fp32_bound`` uses r + 2 for the same sum), the mean's addition rounds once
  more at the size |rec| + |mean|, and the product with ``scale`` once more at the size of the result:
      |out^_d - out_d| <= |scale| (r + 2 + [mean]) u' (sum_i |U_di| |c_i| + |mean_d|) + u |out_d|
  with u' = u / (1 - (r + 3) u).  k + nl = 0 has no arithmetic but the last product: the result is mean * scale or zeros.

``recon_error``:  the six numbers of diagnostics.py:72-117 on rec = U c (+ mean), through ``helpers.diag_check`` /
  ``helpers.diag_fp32_bound`` (which take ``mean=``): the error vector inherits the reconstruction's bound, the five sums
  run in fp64, and the norms are reported as fp32 values (relative 2e-6 covers that and the one rounding of
  ``e = x - rec``).  The given-reconstruction form has no chain at all: ``helpers.diag_check_given``.

Non-finite operands: the expected PATTERN (which of the six numbers are NaN, +Inf, -Inf) is what torch on the CPU gives
for diagnostics.py:72-117 on the same fp32 operands (``oracle.reconstruction_error``); the numbers that stay finite
stay inside the bound.
"""
import math

import numpy as np
import torch

from helpers import diag_fp32_bound

U32 = 2.0 ** -24
U64 = 2.0 ** -53
THREADS = 256
ROWS_PER_BLOCK = 2048
MAX_BLOCKS = 1024

ROWS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]
ROWS_HUGE = [MAX_BLOCKS * ROWS_PER_BLOCK, MAX_BLOCKS * ROWS_PER_BLOCK + 1]      # a ninth row per thread starts here
PAIRS_SMALL = [(k, r - k) for r in range(1, 5) for k in range(r + 1)]            # every pair with 1 <= k + nl <= 4
PAIRS_WIDE = [(0, 32), (32, 0), (1, 31), (31, 1), (16, 16), (7, 9)]
PAIRS = PAIRS_SMALL + PAIRS_WIDE
SPIKE = 1e3                     # times the typical magnitude
TYPICAL = {"U": 0.05, "mean": 0.01, "orig": 0.02}
KEYS = ("absolute_error", "relative_error", "max_absolute_error", "mean_absolute_error", "original_norm",
        "reconstructed_norm")


def grid(rows):
    return max(1, min(MAX_BLOCKS, -(-rows // ROWS_PER_BLOCK)))


def rows_per_thread(rows):
    return -(-rows // (grid(rows) * THREADS))


def spike_rows(rows):
    return sorted({s for s in (0, 255, 256, 2047, 2048, rows - 1) if 0 <= s < rows})


class Case:
    """Seeded operands of one (rows, k, nl, element type): a random basis that is NOT orthonormal, mean, orig, delta
    and coefficients as CPU tensors, with a spike of 1e3 x the typical magnitude in U, mean, orig and delta at the first
    and last row of a thread's first visit (0, 255), of its second (256), of the first block (2047), the second block's
    first row (2048) and the tensor's last row -- different at every spiked row and column, so that neither a swapped
    row nor a swapped column passes for its neighbour."""

    def __init__(self, rows, k, nl, fp16, seed=0):
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 101 * k + nl + (50021 if fp16 else 0))
        r = k + nl
        self.rows, self.k, self.nl, self.r, self.fp16 = rows, k, nl, r, fp16
        U = TYPICAL["U"] * torch.randn(rows, r, generator=g)
        self.mean = TYPICAL["mean"] * torch.randn(rows, generator=g)
        self.orig = TYPICAL["orig"] * torch.randn(rows, generator=g)
        self.delta = TYPICAL["orig"] * torch.randn(rows, generator=g)
        self.coef = torch.randn(r, generator=g)
        for q, s in enumerate(spike_rows(rows)):
            sign = -1.0 if q % 2 else 1.0
            U[s] = sign * SPIKE * TYPICAL["U"] * (1.0 + 0.03 * torch.arange(r) + 0.01 * q)
            self.mean[s] = -sign * SPIKE * TYPICAL["mean"] * (1.0 + 0.07 * q)
            self.orig[s] = sign * SPIKE * TYPICAL["orig"] * (1.0 + 0.05 * q)
            self.delta[s] = sign * SPIKE * TYPICAL["orig"] * (1.0 + 0.11 * q)
        dt = torch.float16 if fp16 else torch.float32
        self.U_high = U[:, :k].to(dt).contiguous()
        self.U_low = U[:, k:].to(dt).contiguous()

    # the operands as the kernels see them: fp64 copies of the stored numbers
    def U64(self):
        return torch.cat([self.U_high.double(), self.U_low.double()], dim=1)

    def c_high(self):
        return self.coef[:self.k]

    def c_low(self):
        return self.coef[self.k:]


# ------------------------------------------------------------------------------------------------ exact values and bounds
def project_exact(U_high, U_low, delta, mean=None):
    """(c [r], bound [r]) of ``svdq_project`` in fp64 on the stored values."""
    rows = delta.numel()
    U = torch.cat([U_high.double(), U_low.double()], dim=1)
    x = delta.double().reshape(-1) - (mean.double().reshape(-1) if mean is not None else 0.0)
    c = U.T @ x
    A = U.abs().T @ x.abs()
    m = rows_per_thread(rows)
    g = (m + 2) * U32 / (1.0 - (m + 2) * U32)
    T = 8 + grid(rows)
    g64 = T * U64 / (1.0 - T * U64)
    E = (g + g64 * (1.0 + g)) * A
    return c, E + U32 * (c.abs() + E)


def reconstruct_exact(U_high, U_low, coef, mean=None, scale=1.0):
    """(out [rows], bound [rows]) of ``svdq_reconstruct`` in fp64 on the stored values; ``scale`` is the fp32 number the
    kernel is handed."""
    U = torch.cat([U_high.double(), U_low.double()], dim=1)
    r = U.shape[1]
    c = coef.double().reshape(-1)
    s = float(np.float32(scale))
    v = U @ c
    A = U.abs() @ c.abs()
    n = r + 2
    if mean is not None:
        v = v + mean.double().reshape(-1)
        A = A + mean.double().abs().reshape(-1)
        n += 1
    out = v * s
    g = n * U32 / (1.0 - (r + 3) * U32)
    return out, abs(s) * g * A + U32 * out.abs()


def six_want(x, U_high, U_low, c_high, c_low, mean=None, recon=None, dtype=torch.float64):
    """The six numbers in ``dtype``: of the fused form (rec = U c (+ mean)), or of a given reconstruction."""
    from oracle import svd_hybrid_oracle as orc
    if recon is not None:
        return orc.reconstruction_error(x.reshape(-1).to(dtype), recon.reshape(-1).to(dtype))
    return orc.parameter_task_diagnostics(x, U_high, U_low, c_high, c_low, dtype=dtype, mean=mean)


def six_ratio(got, x, U_high, U_low, c_high, c_low, mean=None, recon=None):
    """error / tolerance of each of the six numbers under exactly ``helpers.diag_check``'s (``diag_check_given``'s)
    tolerance -- for the mutation proofs and the headroom measurement, which need a figure rather than an assertion."""
    want = six_want(x, U_high, U_low, c_high, c_low, mean=mean, recon=recon)
    tol = {k: 0.0 for k in KEYS} if recon is not None else diag_fp32_bound(U_high, U_low, c_high, c_low, x, mean=mean)
    return {k: abs(float(got[k]) - float(want[k])) / (2e-6 * abs(float(want[k])) + tol[k] + 1e-30) for k in KEYS}


def classify(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("+inf" if v == math.inf else ("-inf" if v == -math.inf else "finite"))


def check_six_nonfinite(got, x, U_high, U_low, c_high, c_low, mean=None, recon=None, what=""):
    """Operands that hold a NaN or an Inf: every number has the class (NaN / +Inf / -Inf / finite) torch gives in fp32
    on the CPU, and the finite ones are inside the bound of the finite rows.  Returns the pattern."""
    want32 = six_want(x, U_high, U_low, c_high, c_low, mean=mean, recon=recon, dtype=torch.float32)
    want64 = six_want(x, U_high, U_low, c_high, c_low, mean=mean, recon=recon)
    tol = {k: 0.0 for k in KEYS}
    if recon is None:      # the bound of the reconstructed norm needs no finite x
        tol = diag_fp32_bound(U_high, U_low, c_high, c_low, torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), mean=mean)
    pattern = {}
    for k in KEYS:
        pattern[k] = classify(want32[k])
        assert classify(got[k]) == pattern[k], (what, k, float(got[k]), "torch (fp32, CPU):", float(want32[k]))
        if pattern[k] == "finite":
            w = float(want64[k])
            assert abs(float(got[k]) - w) <= 2e-6 * abs(w) + tol[k] + 1e-30, (what, k, float(got[k]), w, tol[k])
    return pattern


# ------------------------------------------------------------------------------------------------ fp32 evaluations
ORDERS = ("kernel", "forward", "pairwise")


def _f32(t):
    return np.ascontiguousarray(t.detach().to(torch.float32).numpy())      # exact from fp16


def _fma(a, b, c):
    """fp32 fma through fp64: the product of two fp32 numbers is exact there and the sum rounds at 2^-53 before it
    rounds at 2^-24 -- a legitimate fp32 evaluation inside the bound (the spare rounding of the +2 holds it)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _pairwise(p):
    """fp32 pairwise sum over axis 0."""
    while p.shape[0] > 1:
        if p.shape[0] % 2:
            p = np.concatenate([p, np.zeros_like(p[:1])], axis=0)
        p = (p[0::2] + p[1::2]).astype(np.float32)
    return p[0]


def project_fp32(case, use_mean, order):
    """``svdq_project`` evaluated in fp32 on the kernel's partition of the rows over threads, the thread's sum in one
    of three orders: 'kernel' (a chain of fmas over its rows g, g + stride, ...), 'forward' (product, then addition, in
    that order of rows, no fma) and 'pairwise' (products summed pairwise); fp64 over the threads, one cast at the end."""
    rows, r = case.rows, case.r
    stride, m = grid(rows) * THREADS, rows_per_thread(rows)
    U = np.concatenate([_f32(case.U_high), _f32(case.U_low)], axis=1)
    x = _f32(case.delta)
    if use_mean:
        x = (x - _f32(case.mean)).astype(np.float32)
    pad = m * stride - rows
    U = np.concatenate([U, np.zeros((pad, r), np.float32)]).reshape(m, stride, r)
    x = np.concatenate([x, np.zeros(pad, np.float32)]).reshape(m, stride, 1)
    if order == "kernel":
        acc = np.zeros((stride, r), np.float32)
        for j in range(m):
            acc = _fma(U[j], x[j], acc)
    elif order == "forward":
        acc = np.zeros((stride, r), np.float32)
        for j in range(m):
            acc = (acc + (U[j] * x[j]).astype(np.float32)).astype(np.float32)
    else:
        acc = _pairwise((U * x).astype(np.float32))
    return acc.astype(np.float64).sum(axis=0).astype(np.float32)


def _rec_fp32(case, use_mean, order):
    """The reconstruction's rows in fp32: 'kernel' (two fma chains, high and low, joined by one addition), 'forward' (one
    chain over the r columns without fma), 'pairwise'."""
    Uh, Ul, c = _f32(case.U_high), _f32(case.U_low), _f32(case.coef)
    k, r = case.k, case.r
    if order == "kernel":
        hi = np.zeros(case.rows, np.float32)
        lo = np.zeros(case.rows, np.float32)
        for i in range(k):
            hi = _fma(Uh[:, i], c[i], hi)
        for j in range(r - k):
            lo = _fma(Ul[:, j], c[k + j], lo)
        rec = (hi + lo).astype(np.float32)
    else:
        p = (np.concatenate([Uh, Ul], axis=1) * c[None, :]).astype(np.float32).T      # [r, rows]
        if order == "forward":
            rec = np.zeros(case.rows, np.float32)
            for i in range(r):
                rec = (rec + p[i]).astype(np.float32)
        else:
            rec = _pairwise(p) if r else np.zeros(case.rows, np.float32)
    if use_mean:
        rec = (rec + _f32(case.mean)).astype(np.float32)
    return rec


def reconstruct_fp32(case, use_mean, scale, order):
    return (_rec_fp32(case, use_mean, order) * np.float32(scale)).astype(np.float32)


def six_from(rec32, x32):
    """The six numbers from fp32 rows the way the kernels finish them: e = x - rec in fp32, sums in fp64, norms and the
    mean reported as fp32 values."""
    e = (x32 - rec32).astype(np.float32).astype(np.float64)
    en, on = float(np.float32(math.sqrt(float((e * e).sum())))), float(np.float32(np.linalg.norm(x32.astype(np.float64))))
    return {"absolute_error": en, "relative_error": en / on if on > 1e-10 else 0.0,
            "max_absolute_error": float(np.abs(e).max()), "mean_absolute_error": float(np.float32(np.abs(e).mean())),
            "original_norm": on, "reconstructed_norm": float(np.float32(np.linalg.norm(rec32.astype(np.float64))))}


def six_fp32(case, use_mean, order):
    return six_from(_rec_fp32(case, use_mean, order), _f32(case.orig))


# ------------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("drop_row", "double_row", "split", "no_mean", "mean_after_scale", "stride")


def _read(flat, rows, cols, stride):
    """[rows, cols] read from the flat stored array at ``d * stride + i`` (wrapping at its end, where a kernel would
    read its neighbour's memory)."""
    if cols == 0:
        return torch.zeros(rows, 0, dtype=torch.float64)
    idx = (torch.arange(rows)[:, None] * stride + torch.arange(cols)[None, :]) % flat.numel()
    return flat.double()[idx]


def mutated_basis(case, mutation):
    """[U_high | U_low] in fp64 as a kernel with ``mutation`` reads it.  'split': the k / nl split off by one (one
    column less from U_high's memory, one more from U_low's; needs k >= 1 and nl >= 1).  'stride': row d of U_high read
    with stride k + 1 (needs k >= 1)."""
    k, nl, rows = case.k, case.nl, case.rows
    fh, fl = case.U_high.reshape(-1), case.U_low.reshape(-1)
    if mutation == "split":
        assert k >= 1 and nl >= 1
        return torch.cat([_read(fh, rows, k - 1, k - 1), _read(fl, rows, nl + 1, nl + 1)], dim=1)
    if mutation == "stride":
        assert k >= 1
        return torch.cat([_read(fh, rows, k, k + 1), _read(fl, rows, nl, nl)], dim=1)
    return case.U64()


def project_mutated(case, mutation, row=None):
    """What ``svdq_project`` (with the mean) would return, exactly, had it the mistake ``mutation``; ``row`` is the
    spiked row a dropped / doubled visit concerns."""
    U = mutated_basis(case, mutation)
    x = case.delta.double() - (case.mean.double() if mutation != "no_mean" else 0.0)
    w = torch.ones(case.rows, dtype=torch.float64)
    if mutation == "drop_row":
        w[row] = 0.0
    if mutation == "double_row":
        w[row] = 2.0
    return U.T @ (w * x)


def rec_mutated(case, mutation, row=None, scale=1.0, use_mean=True):
    """The rows ``svdq_reconstruct`` would write (and ``svdq_recon_error`` would compare) under ``mutation``.  A dropped
    row is never written (0) / never compared (its value stands in for the original's, see ``six_mutated``); a doubled
    row is row ``row``'s result written to its neighbour as well; 'mean_after_scale' is (U c) * scale + mean."""
    U = mutated_basis(case, mutation)
    s = float(np.float32(scale))
    v = U @ case.coef.double()
    mu = case.mean.double() if (use_mean and mutation != "no_mean") else torch.zeros(case.rows, dtype=torch.float64)
    out = v * s + mu if mutation == "mean_after_scale" else (v + mu) * s
    if mutation == "drop_row":
        out[row] = 0.0
    if mutation == "double_row":
        out[row + 1 if row + 1 < case.rows else row - 1] = out[row]
    return out


def six_mutated(case, mutation, row=None, use_mean=True):
    """The six numbers (fp64) ``svdq_recon_error`` would report under ``mutation``: a dropped row is left out of every
    sum, a doubled one is counted twice."""
    rec = rec_mutated(case, mutation if mutation not in ("drop_row", "double_row") else None, use_mean=use_mean)
    x = case.orig.double()
    w = torch.ones(case.rows, dtype=torch.float64)
    if mutation == "drop_row":
        w[row] = 0.0
    if mutation == "double_row":
        w[row] = 2.0
    e = x - rec
    en, on = math.sqrt(float((w * e * e).sum())), math.sqrt(float((w * x * x).sum()))
    return {"absolute_error": en, "relative_error": en / on if on > 1e-10 else 0.0,
            "max_absolute_error": float((e.abs() * (w > 0)).max()), "mean_absolute_error": float((w * e.abs()).sum()) / case.rows,
            "original_norm": on, "reconstructed_norm": math.sqrt(float((w * rec * rec).sum()))}
