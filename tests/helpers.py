"""Shared helpers for the test-suite (fixture loading, sign alignment, comparisons)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def bits_equal(a, b):
    """Bit-for-bit equality of two float arrays (NaN == NaN, -0.0 != +0.0)."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    w = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    av, bv = a.view(w), b.view(w)
    if np.array_equal(av, bv):
        return True
    nan_both = np.isnan(a) & np.isnan(b)
    return bool(np.all((av == bv) | nan_both))


def align_signs(U, U_ref):
    """Per-column sign s_j = sign(<u_j, uref_j>); returns (U * s, s). Singular vectors are
    defined up to sign (and up to rotation inside equal-sigma clusters, which callers avoid)."""
    U = np.asarray(U, dtype=np.float64)
    U_ref = np.asarray(U_ref, dtype=np.float64)
    s = np.sign((U * U_ref).sum(axis=0))
    s[s == 0] = 1.0
    return U * s, s


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def as_tensors(arr2d):
    return [torch.from_numpy(np.ascontiguousarray(r)) for r in arr2d]


def _tree(o):
    """Structure of a saved object: key trees, tensor dtypes / shapes, python types (no values)."""
    if isinstance(o, torch.Tensor):
        return {"tensor": str(o.dtype).replace("torch.", ""), "shape": list(o.shape), "device": o.device.type}
    if isinstance(o, torch.Size):
        return {"torch.Size": list(o)}
    if isinstance(o, dict):
        return {"dict": {str(k): _tree(v) for k, v in o.items()}}
    if isinstance(o, (list, tuple)):
        return {type(o).__name__: [_tree(v) for v in o]}
    return type(o).__name__


def _json_tree(o):
    if isinstance(o, dict):
        return {k: _json_tree(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_json_tree(v) for v in o]
    return type(o).__name__


def artifact_manifest(root):
    """Same definition as tests/golden/make_golden.py::artifact_manifest (which applied it to the files the
    reference's writer produced): relative file names, and per file the key tree with dtypes and shapes (.pt, loaded
    weights-only) or the key tree with value types (.json)."""
    import json
    man = {}
    for dirpath, _, files in os.walk(root):
        for f in sorted(files):
            full = os.path.join(dirpath, f)
            rel = os.path.relpath(full, root).replace(os.sep, "/")
            if f.endswith(".pt"):
                man[rel] = _tree(torch.load(full, map_location="cpu", weights_only=True))
            elif f.endswith(".json"):
                man[rel] = _json_tree(json.load(open(full)))
    return man


def diag_fp32_bound(U_high, U_low, c_high, c_low, x, mean=None):
    """Forward-error bound of the fp32 arithmetic in ``U_high.float() @ c_high + U_low.float() @ c_low`` (reference
    diagnostics.py:210-212) for each of the six error numbers: every element of the reconstruction carries at most
    ``(r + 2) * 2^-24 * (|U| |c|)_i`` of rounding whatever order an fp32 implementation sums the r products in (the
    reference's BLAS, a chain of fmas, an MFMA), and the error vector inherits it.  Measured on tests/golden/diag.npz:
    the reference's OWN fp32 numbers sit up to 7e-5 (max_absolute_error, uncentred runs whose error is ~1e-3 of the
    tensor) from the fp64 evaluation of the same formula on the same stored numbers -- inside this bound, far outside
    a flat 1e-5.  Returns {key: absolute tolerance against the fp64 evaluation}."""
    import torch
    A = torch.cat([U_high.double().abs(), U_low.double().abs()], dim=1) @ torch.cat(
        [c_high.double().abs().reshape(-1), c_low.double().abs().reshape(-1)])
    r = U_high.shape[1] + U_low.shape[1]
    if mean is not None:      # the add_mean extension rounds once more, at the size of |rec| + |mean|
        A = A + mean.double().abs().reshape(-1)
        r += 1
    g = (r + 2) * 2.0 ** -24
    xn = float(x.double().norm())
    l2, linf, l1 = float(A.norm()) * g, float(A.max()) * g if A.numel() else 0.0, float(A.mean()) * g if A.numel() else 0.0
    return {"absolute_error": l2, "relative_error": l2 / xn if xn > 1e-10 else 0.0, "max_absolute_error": linf,
            "mean_absolute_error": l1, "original_norm": 0.0, "reconstructed_norm": l2}


def diag_check(got, x, U_high, U_low, c_high, c_low, what="", mean=None, slack=1.0):
    """All six numbers of one (parameter, task) against diagnostics.py:186-215 evaluated in fp64 on the SAME stored
    artifacts (no basis freedom): relative 2e-6 (the fp32 conversion of the norms the kernels report) plus the fp32
    bound above."""
    from oracle import svd_hybrid_oracle as orc
    import torch
    want = orc.parameter_task_diagnostics(x, U_high, U_low, c_high, c_low, dtype=torch.float64, mean=mean)
    tol = diag_fp32_bound(U_high, U_low, c_high, c_low, x, mean=mean)
    for key in orc.DIAG_KEYS:
        g, w = float(got[key]), float(want[key])
        assert abs(g - w) <= 2e-6 * abs(w) + slack * tol[key] + 1e-30, (what, key, g, w, tol[key])


def diag_check_given(got, x, recon, what=""):
    """The six numbers of a GIVEN reconstruction (diagnostics.py:72-117 on two tensors): there is no chain of products
    to bound, ``e = x - recon`` rounds once (relative 2^-24 per element, so at most that on each norm, the maximum and
    the mean) and the norms are reported as fp32 values -- relative 2e-6 holds both."""
    from oracle import svd_hybrid_oracle as orc
    want = orc.reconstruction_error(x.reshape(-1).double(), recon.reshape(-1).double())
    for key in orc.DIAG_KEYS:
        g, w = float(got[key]), float(want[key])
        assert abs(g - w) <= 2e-6 * abs(w) + 1e-30, (what, key, g, w)


def diag_check_chunked(got, x, U_high, U_low, c_high, c_low, what="", chunk=1 << 24):
    """diag_check for tensors too long for one library call (2^30 rows: a single fp64 matrix-vector product of that
    length is itself suspect): the same formula and the same bound, accumulated over row chunks in fp64."""
    import math
    import torch
    c = torch.cat([c_high.double().reshape(-1), c_low.double().reshape(-1)])
    ca = c.abs()
    D = x.numel()
    se = sx = sr = sa = mx = a2 = a1 = amax = 0.0
    for lo in range(0, D, chunk):
        sl = slice(lo, min(lo + chunk, D))
        U = torch.cat([U_high[sl].double(), U_low[sl].double()], dim=1)
        rec = (U * c).sum(dim=1)      # elementwise: a library matrix-vector product refuses / mishandles this many rows
        xs = x[sl].double().reshape(-1)
        e = xs - rec
        A = (U.abs() * ca).sum(dim=1)
        se += float((e * e).sum()); sx += float((xs * xs).sum()); sr += float((rec * rec).sum())
        sa += float(e.abs().sum()); mx = max(mx, float(e.abs().max()))
        a2 += float((A * A).sum()); a1 += float(A.sum()); amax = max(amax, float(A.max()))
    g = (U_high.shape[1] + U_low.shape[1] + 2) * 2.0 ** -24
    xn = math.sqrt(sx)
    want = {"absolute_error": math.sqrt(se), "relative_error": math.sqrt(se) / xn if xn > 1e-10 else 0.0,
            "max_absolute_error": mx, "mean_absolute_error": sa / D, "original_norm": xn, "reconstructed_norm": math.sqrt(sr)}
    tol = {"absolute_error": math.sqrt(a2) * g, "relative_error": math.sqrt(a2) * g / xn if xn > 1e-10 else 0.0,
           "max_absolute_error": amax * g, "mean_absolute_error": a1 / D * g, "original_norm": 0.0,
           "reconstructed_norm": math.sqrt(a2) * g}
    for key, w in want.items():
        assert abs(float(got[key]) - w) <= 2e-6 * abs(w) + tol[key] + 1e-30, (what, key, float(got[key]), w, tol[key])


# ------------------------------------------------------------------------------------------------ the device's own artifacts
def check_pipeline_quantizer(orc, plan, sm, p):
    """Kernel-level parity of the in-pipeline (one lane per task) quantizer: the oracle applied to
    OUR fp32 coefficients must give OUR codes / scale / zero_point bit for bit, inf and NaN included."""
    k, r = int(sm.k[p]), int(sm.r[p])
    nl = r - k
    for t in range(plan.N):
        want = orc.rtvq_quantize(sm.coef[p, t, k:r], plan.bits, plan.S)
        if nl == 0:
            continue
        assert np.array_equal(sm.codes[p, t, :, :nl], want["codes"]), (p, t)
        assert bits_equal(sm.scale[p, t], want["scale"]), (p, t, sm.scale[p, t], want["scale"])
        assert bits_equal(sm.zero_point[p, t], want["zero_point"]), (p, t)
        np.testing.assert_allclose(sm.residual_norm[p, t], want["residual_norm"], rtol=1e-5, equal_nan=True)
        c16 = torch.from_numpy(sm.coef[p, t, :k].copy()).half().numpy()
        assert np.array_equal(sm.c_high[p, t, :k].view(np.uint16), c16.view(np.uint16))


def own_basis(plan, p, k, r, D):
    """The stored basis [U_high | U_low] of parameter ``p`` as an fp64 array [D, r] and the stored mean as fp32 [D]
    (None on an uncentred plan): what ``own_projection_mismatch`` projects on."""
    Uh, Ul, mu = plan.basis_tensors(p, k, r, D)
    U = torch.cat([Uh, Ul], dim=1).double().cpu().numpy() if (k > 0 and r > k) else \
        (Uh if k > 0 else Ul).double().cpu().numpy()
    return U, (mu.flatten().cpu().numpy() if mu is not None else None)


def own_projection_mismatch(U, mu32, delta, got, sigma, t=0):
    """Projection on the device's own basis: the coefficients of task ``t`` (``got``, fp32 [r]) against
    ``U^T (delta - mean)`` in fp64 on the host, with ``U`` / ``mu32`` from ``own_basis`` -- free of the basis freedom
    (signs, rotations inside near-degenerate subspaces).  Returns None, or the mismatch as a message."""
    r = U.shape[1]
    x32 = delta.numpy() - mu32 if mu32 is not None else delta.numpy()      # fp32, like compress.py:44
    want = U.T @ x32.astype(np.float64)
    got = np.asarray(got).astype(np.float64)
    # column i is U_i = Tc v_i / sigma_i formed in fp32: its own error is ~eps32 sigma_0 / sigma_i, and the
    # coefficient (closed form sigma_i v_i + the fp16-rounding correction) differs from the explicit projection
    # on the stored column by that much of |x| (seed 5001 case 805: sigma_30 = 5e-4 sigma_0, 3e-5 |x|)
    # The model has no ceiling of its own: round 3 had capped it at 1e-3 |x| by hand, which a direction at
    # 1.9e-6 sigma_0 -- above the 1e-6 null threshold, below the 1e-5 floor under which not even singular values
    # are compared; its fp32-formed column is only ~97 % the singular vector -- exceeded with 1.75e-3 |x| (seed 4
    # case 37: D = 31 < N = 32; model: 0.16 |x|).  Capped where the model reaches 1e-2 (sigma_i = 3e-5 sigma_0);
    # such a direction holds < 1e-9 of the energy and the reconstructions still agree to MSE 3e-10.
    sg = np.maximum(np.asarray(sigma)[:r].astype(np.float64), 1e-30)
    tol = float(np.linalg.norm(x32)) * np.minimum(1e-5 + 3e-7 * sg[0] / sg, 1e-2) + 1e-12
    if mu32 is not None:      # the rows of T - mean sum to a few ulp(mean), not to 0; the device removes that
        tol = tol + 2.4e-7 * float(np.linalg.norm(mu32))      # component (1 / sqrt(N) is deflated), a GEMV keeps it
    if np.isfinite(want).all() and not np.all(np.abs(got - want) <= tol):
        bad_i = int(np.argmax(np.abs(got - want) / tol))
        return (f"projection on the device's basis: task {t} column {bad_i}, |dc| "
                f"{abs(got[bad_i] - want[bad_i]):.2e} (tol {tol[bad_i]:.1e})")
    return None


# ------------------------------------------------------------------------------------------------ basis rows
# The constants of basis_rows_ratios that cannot be derived to the last factor.  Fitted on the REFERENCE chain on the CPU
# (oracle.svd_basis + oracle.project: LAPACK fp32 SVD, .half(), fp32 GEMVs) over every (N, D, centre, storage, unit
# size) of tests/test_hip_basis_rows.py -- 3 200 chains up to D = 70 001 and the four of D = 4 194 307 -- as TWICE the
# largest value any chain needs; tools/fit_basis_rows.py regenerates the figures, DESIGN.md section 2 has the table.
# Never tuned on the kernels.
#   g: coefficient term of identity (a).  What the reference needs grows with D as the error of a D-term fp32 product
#      does -- fp32 basis: 88 at D = 256, 305 at 8 193, 523 at 70 001, 7 470 at 4 194 307, i.e. 2 ... 5.51 sqrt(D), the
#      largest at D = 256, N = 2 -- so g = BASIS_ROWS_G sqrt(D) from BASIS_ROWS_SMALL rows on.  Below, sqrt(D) means
#      nothing (D = 4, N = 3, centred needs 24.32 = 12.16 sqrt(D)) and g is the flat BASIS_ROWS_G0.  fp16 basis: 0 up to
#      D = 70 001 (the two u terms cover it), 3.26 sqrt(D) at D = 4 194 307 (N = 32, uncentred).
#   c: fp32 term of identity (c).  Needed: 17.0 up to D = 70 001, 140.5 at D = 4 194 307 (N = 16: LAPACK's
#      |U^T U - I| reaches 1.0e-5 there).  The rounding to fp16 happens to a column formed in fp32, so the term applies
#      under both storage types; the fp16 reference alone needs none (its |U^T U - I| <= 6.3e-4 is inside the rounding part).
#   The figures of the 4 M-row shapes move with LAPACK's blocking, i.e. with the thread count (measured with 4 threads;
#   smaller needs have been seen with 16); those up to D = 70 001 do not.
BASIS_ROWS_SMALL = 64
BASIS_ROWS_G0 = {True: 0.0, False: 2 * 24.32}
BASIS_ROWS_G = {True: 2 * 3.26, False: 2 * 5.51}
BASIS_ROWS_C = {True: 2 * 140.5, False: 2 * 140.5}
NULL_SIGMA = 1e-6        # sigma_j <= NULL_SIGMA sigma_0: a null direction ("Null directions")


def basis_rows_ratios(deltas, U_high, U_low, mean, coef, sigma, fp16, center, g0=None, g=None, c=None, chunk=1 << 18):
    """The three row-local identities of the compressor's streaming outputs, in fp64 on the host, from the original
    fp32 inputs: ``deltas`` (N tensors of >= D elements), ``U_high [D, k]`` / ``U_low [D, r-k]`` / ``mean [D, 1] | None``
    as stored, ``coef [N, r]`` the fp32 coefficients before rounding and ``sigma [r]`` the reported singular values.
    Evaluated in row chunks, so host memory stays flat.  Returns error / bound ratios and what a fit needs:

    (a) |T[i,t] - mean[i] - sum_j U[i,j] coef[t,j]| per ELEMENT against
          u A_it + [fp16: 2^-25 sum_j |c_tj|]                      storage rounding of U (u = 2^-11 fp16, 2^-24 fp32)
        + (r + N) 2^-24 (A_it + sum_t |T_it| + |mean_i|)           fp32 arithmetic of the row; A = |U| |c|^T
        + sum_j |U_ij| (u + g 2^-24) (|U_j|^T |Tc_t|)              a coefficient on the stored column: projection of the
                                                                   storage error + the fp32 error of a D-term product
                                                                   (g = G0 for D < 64, G sqrt(D) from there on)
        + sum over zero columns j of sigma64_j                     a null direction is left out by design
        + 1e-30
    (b) |mean[i] - mean64[i]| <= (N + 1) 2^-24 sum_t |T_it| / N
    (c) |U^T U - I| per entry over the nonzero columns against
          [fp16: (2u + u^2) (|U|^T |U|)_ij + 2^-25 (1 + u) (|U_i|_1 + |U_j|_1) + D 2^-50]     rounding of both factors
        + c 2^-24 sigma_0 / min(sigma_i, sigma_j)                  a column formed in fp32
        with sigma = the fp64 singular values of the (centred) INPUT, a null direction's nonzero column (the completion,
        or whatever LAPACK returns there) taking the smallest real sigma.  A column is exactly zero or subject to this;
        zero only where sigma64_j <= 2e-6 sigma64_0 and the reported sigma_j <= 1e-6 sigma_0.
    """
    N = len(deltas)
    D = int(U_high.shape[0])
    r = int(U_high.shape[1] + U_low.shape[1])
    assert (mean is None) == (not center), "mean must be None exactly when centring is off"
    assert U_low.shape[0] == D and all(d.numel() >= D for d in deltas)
    C = torch.as_tensor(np.ascontiguousarray(np.asarray(coef)[:N, :r], dtype=np.float64)).reshape(N, r)
    Ca = C.abs()
    e32 = 2.0 ** -24
    u = 2.0 ** -11 if fp16 else e32
    floor = 2.0 ** -25 if fp16 else 0.0
    if D < BASIS_ROWS_SMALL:
        gk = BASIS_ROWS_G0[bool(fp16)] if g0 is None else g0
    else:
        gk = (BASIS_ROWS_G[bool(fp16)] if g is None else g) * np.sqrt(D)
    ck = BASIS_ROWS_C[bool(fp16)] if c is None else c
    mflat = mean.reshape(-1) if mean is not None else None
    inf = float("inf")      # a NaN anywhere in the outputs is an error of infinite size, not a comparison that is False

    def rows(lo, hi):
        T = torch.stack([d.reshape(-1)[lo:hi] for d in deltas], dim=1).double()
        U = torch.cat([U_high[lo:hi].double(), U_low[lo:hi].double()], dim=1)
        mu = mflat[lo:hi].double() if center else torch.zeros(hi - lo, dtype=torch.float64)
        return T, U, mu

    # pass 1: the mean, and the column sums that (a) and (c) need
    M = torch.zeros(r, N, dtype=torch.float64)
    G = torch.zeros(r, r, dtype=torch.float64)
    Ga = torch.zeros(r, r, dtype=torch.float64)
    GT = torch.zeros(N, N, dtype=torch.float64)
    l1 = torch.zeros(r, dtype=torch.float64)
    out = {"b": 0.0, "b_row": -1}
    for lo in range(0, D, chunk):
        hi = min(lo + chunk, D)
        T, U, mu = rows(lo, hi)
        m64 = T.mean(dim=1) if center else torch.zeros(hi - lo, dtype=torch.float64)
        if center:
            rb = ((mu - m64).abs() / ((N + 1) * e32 * T.abs().sum(dim=1) / N + 1e-30)).nan_to_num(nan=inf)
            i = int(rb.argmax())
            if float(rb[i]) > out["b"]:
                out["b"], out["b_row"] = float(rb[i]), lo + i
        Ua = U.abs()
        M += Ua.T @ (T - mu[:, None]).abs()
        G += U.T @ U
        Ga += Ua.T @ Ua
        l1 += Ua.sum(dim=0)
        Tc = T - m64[:, None]
        GT += Tc.T @ Tc
    if D <= chunk:
        T = rows(0, D)[0]
        S64 = torch.linalg.svdvals(T - T.mean(dim=1, keepdim=True) if center else T)
    else:      # sigma >= 1e-6 sigma_0 from an fp64 Gram: 1e-16 sigma_0^2 / sigma^2 <= 1e-4 relative
        S64 = torch.linalg.eigvalsh(GT).flip(0).clamp_min(0.0).sqrt()
    S64 = S64[:r].numpy().copy()
    out["S64"] = S64
    s0 = float(S64[0]) if r else 0.0
    zero = (l1 == 0).numpy()
    sg = np.asarray(sigma, dtype=np.float64).reshape(-1)[:r]
    for j in np.nonzero(zero)[0]:
        assert S64[j] <= 2 * NULL_SIGMA * s0 and sg[j] <= NULL_SIGMA * sg[0], \
            f"column {j} is zero but sigma64 = {S64[j]:.3e} (sigma64_0 = {s0:.3e}), reported {sg[j]:.3e}"
    null = float(S64[zero].sum())

    # (c); an all-zero input (sigma_0 = 0) has no direction to hold orthonormal: every column may be zero or the completion
    out.update({"c": 0.0, "c_need": 0.0, "c_at": (-1, -1), "c_err": 0.0})
    nz = np.nonzero(~zero)[0]
    real = S64 > NULL_SIGMA * s0
    if s0 > 0 and nz.size and real.any():
        se = np.maximum(S64, S64[real].min())[nz]
        idx = torch.as_tensor(nz)
        err = (G[idx][:, idx] - torch.eye(nz.size, dtype=torch.float64)).abs().numpy()
        b16 = np.zeros_like(err)
        if fp16:
            l = l1[idx].numpy()
            b16 = (2 * u + u * u) * Ga[idx][:, idx].numpy() + floor * (1 + u) * (l[:, None] + l[None, :]) + D * floor ** 2
        b32 = e32 * s0 / np.minimum.outer(se, se)
        rc = np.nan_to_num(err / (b16 + ck * b32 + 1e-300), nan=inf)
        a = np.unravel_index(int(rc.argmax()), rc.shape)
        out.update({"c": float(rc[a]), "c_at": (int(nz[a[0]]), int(nz[a[1]])), "c_err": float(err.max()),
                    "c_need": float(np.maximum((err - b16) / b32, 0.0).max())})

    # pass 2: (a)
    out.update({"a": 0.0, "a0": 0.0, "a_need": 0.0, "a_at": (-1, -1), "a_err": 0.0, "a_tol": 0.0})
    for lo in range(0, D, chunk):
        hi = min(lo + chunk, D)
        T, U, mu = rows(lo, hi)
        Ua = U.abs()
        E = (T - mu[:, None] - U @ C.T).abs()
        A = Ua @ Ca.T
        L = (u * A + floor * Ca.sum(dim=1)[None, :]
             + (r + N) * e32 * (A + T.abs().sum(dim=1, keepdim=True) + mu.abs()[:, None])
             + u * (Ua @ M) + null + 1e-30)
        Cg = e32 * (Ua @ M)
        ra = (E / (L + gk * Cg)).nan_to_num(nan=inf)
        i = int(ra.argmax())
        if float(ra.reshape(-1)[i]) > out["a"]:
            out.update({"a": float(ra.reshape(-1)[i]), "a_at": (lo + i // N, i % N), "a_err": float(E.reshape(-1)[i]),
                        "a_tol": float((L + gk * Cg).reshape(-1)[i])})
        out["a0"] = max(out["a0"], float((E / L).max()))      # without the g term
        need = ((E - L).clamp_min(0.0) / (Cg + 1e-300)).max()
        out["a_need"] = max(out["a_need"], float(need))
    return out


def basis_rows_assert(s, what=""):
    """The verdict on what basis_rows_ratios returned: each identity's largest error / bound is at most 1."""
    assert s["b"] <= 1.0, (what, "(b) mean", "row", s["b_row"], "error / bound", s["b"])
    assert s["a"] <= 1.0, (what, "(a) row identity", "row, task", s["a_at"], "error", s["a_err"], "bound", s["a_tol"],
                           "error / bound", s["a"])
    assert s["c"] <= 1.0, (what, "(c) orthonormality", "columns", s["c_at"], "max error", s["c_err"], "error / bound", s["c"])


def basis_rows_check(deltas, U_high, U_low, mean, coef, sigma, fp16, center, what="", chunk=1 << 18):
    """Asserts the three identities of basis_rows_ratios with the committed constants; returns the ratios."""
    s = basis_rows_ratios(deltas, U_high, U_low, mean, coef, sigma, fp16, center, chunk=chunk)
    basis_rows_assert(s, what)
    return s


BASIS_ROWS_N = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 19, 20, 21, 24, 27, 28, 31, 32]
BASIS_ROWS_LARGE = [(4 * 2 ** 20 + 3, 8, True, True), (4 * 2 ** 20 + 3, 16, False, True), (4 * 2 ** 20 + 3, 20, True, True),
                    (4 * 2 ** 20 + 3, 32, True, False)]      # (D, N, fp16, center)


def basis_rows_sizes(N):
    """The parameter sizes of one plan: around the task count, the 64-row wave tile, the 256-row block, the 1024- /
    4096- / 8192-row units, several units with a partial last block, and one of many units with an odd tail."""
    return [D for D in (1, 2, N - 1, N, N + 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8193,
                        3 * 8192 + 255, 70001) if D > 0]


def basis_rows_inputs(orc, D, N, unit_rows=0):
    """``synthetic_deltas`` (seeded per (N, D)) plus a spike, different for every task and boundary, at the first and
    last rows of the 64-row tile, the 256-row block and the unit, and at the tensor's last row: those rows differ from
    their neighbours by several times the data (1e-2), so one written to the wrong place cannot pass for its neighbour."""
    ds = [d.clone() for d in orc.synthetic_deltas(D, N, 7919 * N + D, rank=min(3, N))]
    ur = unit_rows or (8192 if N > 16 else 4096)
    for q, row in enumerate((0, 63, 64, 255, 256, ur - 1, ur, D - 1)):
        if 0 <= row < D:
            for t, d in enumerate(ds):
                d[row] += (0.05 + 0.01 * t + 0.003 * q) * (-1.0 if (q + t) % 3 == 0 else 1.0)
    return ds


def reference_chain(orc, deltas, center, fp16):
    """What the kernels replace, on the CPU: LAPACK fp32 SVD, the ``.half()`` cast, fp32 GEMVs against the cast basis.
    Returns (U_high, U_low, mean, coef [N, r], sigma [r])."""
    b = orc.svd_basis(deltas, 0.9, None, center, fp16)
    mean = b["mean"]
    coef = []
    for d in deltas:
        ch, cl = orc.project(d if mean is None else d - mean.squeeze(1), b["U_high"], b["U_low"])
        coef.append(torch.cat([ch, cl]).numpy())
    return b["U_high"], b["U_low"], mean, np.stack(coef), b["singular_values"].numpy()
