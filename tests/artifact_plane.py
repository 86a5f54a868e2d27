"""
The (k, r) plane of a plan's stored artifacts: a builder of plans whose every parameter sits at another point of the
plane, and the fp64 model of what the artifact consumers compute from them.  No GPU code: the GPU tests
(test_hip_artifact_plane.py, test_hip_store_values_plane.py) import the contents, the CPU test
(test_artifact_plane_cpu.py) checks the model and the bound themselves.

The plane.  ``plane(N)`` is the list of (k, r) of one task count: all of 1 <= r <= N, 0 <= k <= r up to 8 tasks; above,
r in {1, N // 2, N - 1, N} crossed with k in {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, r - 1, r} (both sides of the 16-byte
load window at either element size, of the 8- and 16-column marks, and the two ends).  Parameter i of a plan takes
``ROW_EDGES[i % len(ROW_EDGES)]`` rows -- the edges of both block sizes (256 rows up to 16 tasks, 128 above) and five
units at unit_rows = 256 -- and pair ``plane(N)[i % len(plane(N))]``, clamped to r <= rows, k <= r.  There are
max(len(plane(N)), len(ROW_EDGES)) + len(ROW_EDGES) parameters: the plane once (a plane shorter than the row list
going round until every row count is used), then one more turn of the row list, so that odd and even k both meet the
128- and 256-row edges at every task count.  The clamp stays for the 1-, 3- and 13-row parameters, and a pair that
it has taken away at every slot it met is built once more behind them, at the next row count in turn that holds it:
every pair of the plane is built unclamped at least once (test_artifact_plane_cpu.py asserts both).  Six long
parameters (4097 and 8193 rows) and one parameter whose rows_dev is 0 follow.

Contents (tests/test_hip_store_gram.py's ``Store``): U random and NOT orthonormal, entries around 1 / sqrt(rows) plus a
shared component, in the basis dtype; a random mean; random fp16 c_high; codes uniform in [0, 2^bits), scales in
[2, 32], integer zero points in [0, 2^bits): everything finite by construction.  Spikes of 1e3 x the typical magnitude
sit in U and the mean at rows 0, 63, 64, 127, 128, 255, 256 and the last row, another value per column: a dropped,
doubled or shifted row, or a column read from the wrong part, is far outside any rounding bound.

The model.  ``coef`` is one task's coefficient vector exactly as task_coeff (csrc/svdq_merge_stream.h) forms it: column
i < k the fp16 c_high, else 0 + sum over the stages of (q - zero_point) / scale_s -- fp32 operations with one rounding
each, which numpy float32 reproduces bit for bit.  ``cbar`` is k_merge_coeff's acc = acc + c * w, task by task in
``order``, skipping w < 0, the product and the sum rounded separately: again exact.  The rows are then evaluated in fp64:
(U_high c_high + U_low c_low + mean) * scale (+ base), the sets combined as combine_sets does.  Only the fma chains are
not emulated (a double-rounded fp64 emulation of fmaf is not exact); they are what the bound covers.

The bound, per element -- derived, not fitted.  u = 2^-24.
  * A chain of m fused multiply-adds from 0 is within gamma_m <= (m + 2) u of the exact sum relative to sum |U||c|, in
    any order (helpers.diag_fp32_bound uses the same figure).  The two chains of a row have k and r - k steps, so
    hi and lo together carry at most (r + 2) u (|U| |c|)_row.  The fp16 -> fp32 conversions of U and c_high are exact.
  * Every later operation -- hi + lo, + mean, * scale, + base, and per set * share and + -- rounds its result once:
    if the exact operation on the model's running value gives y and the error carried into it is e (an addition
    carries e on, a multiplication by s carries |s| e), the computed operand is within e of y, its rounding moves it by
    at most u (|y| + e), so the error carried out is e + u (|y| + e).
Nothing else enters: the coefficients are exact, and -ffp-contract=off keeps the epilogue's operations apart.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
TASKS = [1, 3, 8, 16, 17, 20, 32]
ROW_EDGES = [1, 3, 13, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 1027]
SPIKE_ROWS = [0, 63, 64, 127, 128, 255, 256]      # + the last row
K_MARKS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
BITS = 4
STAGES = 2
UNIT_ROWS = 256


# ------------------------------------------------------------------------------------------------ the plane
def plane(n):
    """The (k, r) pairs of one task count, r ascending, k ascending inside."""
    if n <= 8:
        return [(k, r) for r in range(1, n + 1) for k in range(r + 1)]
    out = []
    for r in sorted({1, n // 2, n - 1, n}):
        for k in sorted({k for k in K_MARKS + [r - 1, r] if 0 <= k <= r}):
            out.append((k, r))
    return out


def clamp(k, r, rows):
    """r <= rows, k <= r (test_hip_plan_project.py's _kr)."""
    r = min(r, rows)
    return min(k, r), r


def long_pairs(n):
    """(rows, k, r) of the parameters behind the plane: several units, a block's first row anywhere."""
    return [(4097, n - 1, n), (4097, n // 2, n), (4097, 0, n), (4097, n, n), (4097, min(1, n), n), (8193, n - 1, n)]


def parameters(n, zero=True):
    """[(rows, k, r)] of one plan; rows None = the parameter whose rows_dev is 0."""
    pl = plane(n)
    out = []
    for i in range(max(len(pl), len(ROW_EDGES)) + len(ROW_EDGES)):
        rows = ROW_EDGES[i % len(ROW_EDGES)]
        out.append((rows,) + clamp(*pl[i % len(pl)], rows))
    # a pair the clamp has taken away at every slot it met: once more, at the next edge in turn that holds it
    i = len(out)
    for k, r in pl:
        if (k, r) not in {(kk, rr) for _, kk, rr in out}:
            while ROW_EDGES[i % len(ROW_EDGES)] < r:
                i += 1
            out.append((ROW_EDGES[i % len(ROW_EDGES)], k, r))
            i += 1
    out += long_pairs(n)
    if zero:
        out.insert(3, (None, 0, 0))
    return out


def spike_rows(rows):
    return sorted({s for s in SPIKE_ROWS + [rows - 1] if s < rows})


# ------------------------------------------------------------------------------------------------ contents
class Entry:
    """The contents of one parameter: U [rows, r] (torch, the basis dtype), mean [rows] fp32 or None, c_high [N, k] fp16,
    codes [N, S, r - k] uint8, scale / zero_point [N, S] fp32 (numpy)."""

    def __init__(self, rows, k, r, n, stages, bits, fp16, center, g):
        self.rows, self.k, self.r, self.n, self.stages, self.bits = rows, k, r, n, stages, bits
        typ = 1.0 / np.sqrt(rows)
        u = (torch.randn(rows, r, generator=g) + 0.5 * torch.randn(rows, 1, generator=g)) * typ
        m = torch.randn(rows, generator=g) * typ
        for s in spike_rows(rows):
            u[s] = 1.0e3 * typ * (1.0 + 0.25 * torch.rand(r, generator=g))
            m[s] = -1.0e3 * typ * (1.0 + 0.25 * float(torch.rand(1, generator=g)))
        self.U = u.to(torch.float16 if fp16 else torch.float32)
        self.mean = m if center else None
        q = 1 << bits
        self.c_high = torch.randn(n, k, generator=g).numpy().astype(np.float16)
        self.codes = torch.randint(0, q, (n, stages, r - k), generator=g).numpy().astype(np.uint8)
        self.scale = (2.0 + 30.0 * torch.rand(n, stages, generator=g)).numpy().astype(np.float32)
        self.zero_point = torch.randint(0, q, (n, stages), generator=g).numpy().astype(np.float32)
        self.U64 = self.U.double().numpy()
        self.mean64 = None if self.mean is None else self.mean.double().numpy()

    def small(self):
        """The entry ``pipeline.pack_small`` takes."""
        return {"rows": self.rows, "k": self.k, "r": self.r, "energy": 0.5, "sigma": np.ones(self.r, np.float32),
                "c_high": self.c_high, "codes": self.codes, "scale": self.scale, "zero_point": self.zero_point,
                "residual_norm": np.zeros((self.n, self.stages), np.float32)}

    def basis_dict(self):
        """The region's basis dictionary in the layout the artifact files hold."""
        k = self.k
        return {"U_high": self.U[:, :k].contiguous(), "U_low": self.U[:, k:].contiguous(),
                "singular_values": torch.ones(self.r), "k": k,
                "mean": None if self.mean is None else self.mean.clone().reshape(-1, 1), "energy_retained": 0.5,
                "D": self.rows, "N": self.n}

    def task_dict(self, t):
        """Task t's artifact of the region in the same layout."""
        nl = self.r - self.k
        pays = [{"stage": s, "quantized": torch.from_numpy(self.codes[t, s].copy()),
                 "scale": torch.tensor(float(self.scale[t, s]), dtype=torch.float32),
                 "zero_point": torch.tensor(float(self.zero_point[t, s]), dtype=torch.float32), "residual_norm": 0.0}
                for s in range(self.stages)]
        return {"c_high_fp16": torch.from_numpy(self.c_high[t].copy()),
                "c_low_quant": {"payloads": pays, "num_bits": self.bits, "num_stages": self.stages,
                                "original_shape": torch.Size([nl]), "original_dtype": "torch.float32"}}


class Contents:
    """The contents of one plan of the plane: ``entries[p]`` (None = the parameter whose rows_dev is 0), made once from a
    seed and never changed."""

    def __init__(self, n, *, fp16, center, stages=STAGES, bits=BITS, zero=True, params=None, seed=0):
        g = torch.Generator().manual_seed(104729 * n + 2 * seed + int(fp16) + 7 * stages)
        self.n, self.fp16, self.center, self.stages, self.bits = n, fp16, center, stages, bits
        self.params = parameters(n, zero) if params is None else list(params)
        self.entries = [None if rows is None else Entry(rows, k, r, n, stages, bits, fp16, center, g)
                        for rows, k, r in self.params]
        self.rows = [0 if e is None else e.rows for e in self.entries]
        self.plan_rows = [300 if e is None else e.rows for e in self.entries]

    def live(self):
        """[(p, entry)] of the parameters that have rows."""
        return [(p, e) for p, e in enumerate(self.entries) if e is not None]

    def small_entries(self):
        return [None if e is None else e.small() for e in self.entries]

    def dictionaries(self):
        """(names, tasks, bases, compressed) in the reference layout -- bases[name]["masked"] /
        compressed[name][task]["masked"] -- for driver.adopt_artifacts; the parameter without rows has no such form."""
        tasks = [f"t{t:02d}" for t in range(self.n)]
        names, bases, comp = [], {}, {}
        for p, e in self.live():
            name = f"q{p:03d}.r{e.rows:05d}.k{e.k:02d}.r{e.r:02d}"
            names.append(name)
            bases[name] = {"masked": e.basis_dict(), "noise": None}
            comp[name] = {t: {"masked": e.task_dict(i)} for i, t in enumerate(tasks)}
        return names, tasks, bases, comp


# ------------------------------------------------------------------------------------------------ the model
def dequantize(codes, scale, zero_point, stages=None):
    """c_low [n_low] float32 of one task as task_coeff adds it up: 0 + (q - zp) / scale, stage by stage, every operation
    rounded to fp32.  ``stages``: the stages to add (None = all)."""
    c = np.zeros(codes.shape[-1], dtype=np.float32)
    for s in (range(codes.shape[0]) if stages is None else stages):
        d = (codes[s].astype(np.float32) - np.float32(zero_point[s])).astype(np.float32)
        c = (c + (d / np.float32(scale[s])).astype(np.float32)).astype(np.float32)
    return c


def coef(e, t, stages=None):
    """Task t's coefficients [r] float32: the bits task_coeff returns."""
    return np.concatenate([e.c_high[t].astype(np.float32), dequantize(e.codes[t], e.scale[t], e.zero_point[t], stages)])


def coefs(e):
    """[N, r] float32."""
    return np.stack([coef(e, t) for t in range(e.n)])


def cbar(e, weights, order=None, C=None):
    """[S, r] float32: k_merge_coeff's averaged coefficients of the sets ``weights`` [S, N]."""
    C = coefs(e) if C is None else C
    w = np.asarray(weights, dtype=np.float32)
    order = range(e.n) if order is None else [int(t) for t in order]
    out = np.zeros((w.shape[0], e.r), dtype=np.float32)
    for s in range(w.shape[0]):
        acc = np.zeros(e.r, dtype=np.float32)
        for t in order:
            if w[s, t] < 0:
                continue
            acc = (acc + (C[t] * w[s, t]).astype(np.float32)).astype(np.float32)
        out[s] = acc
    return out


def _rounded(y, err):
    """The error carried out of an operation whose exact result on the model's running value is y."""
    return err + U32 * (np.abs(y) + err)


def rows_model(e, C, scale=1.0, U=None, k=None):
    """((hi + lo [+ mean]) * scale in fp64, its bound) for the coefficient vectors C [S, r]: both [rows, S]."""
    U = e.U64 if U is None else U
    c = np.asarray(C, dtype=np.float32).astype(np.float64)
    sc = float(np.float32(scale))
    y = U @ c.T
    err = (e.r + 2) * U32 * (np.abs(U) @ np.abs(c).T)
    err = _rounded(y, err)                      # hi + lo
    if e.mean64 is not None:
        y = y + e.mean64[:, None]
        err = _rounded(y, err)                  # + mean
    y = y * sc
    err = _rounded(y, err * abs(sc))            # * scale
    return y, err


def _based(y, err, base):
    if base is None:
        return y, err
    y = y + np.asarray(base, dtype=np.float32).astype(np.float64).reshape(-1, *([1] * (y.ndim - 1)))
    return y, _rounded(y, err)                  # + base


def task_rows(e, scale=1.0, base=None, C=None):
    """(values, bound) [rows, N] fp64 of every task of the parameter: (U_high c_high + U_low c_low + mean) * scale
    (+ base)."""
    y, err = rows_model(e, coefs(e) if C is None else C, scale)
    return _based(y, err, base)


def task_values(e, t, scale=1.0, base=None):
    """Task t's values [rows] fp64."""
    return task_rows(e, scale, base, C=coef(e, t)[None])[0][:, 0]


def merged_rows(e, weights, order=None, set_share=None, scale=1.0, base=None):
    """(values, bound) [rows] fp64 of the merge of the sets ``weights`` [S, N]: the row of every set on its averaged
    coefficients, the sets combined as combine_sets does (res = res + v * share, set by set over share >= 0; without a
    share table the row of set 0), + base."""
    y, err = rows_model(e, cbar(e, weights, order), scale)
    if set_share is None:
        res, eres = y[:, 0], err[:, 0]
    else:
        sh = np.asarray(set_share, dtype=np.float32).astype(np.float64)
        res, eres = np.zeros(e.rows), np.zeros(e.rows)
        for s in range(sh.size):
            if sh[s] < 0:
                continue
            p = y[:, s] * sh[s]
            ep = _rounded(p, err[:, s] * abs(sh[s]))      # * share
            res = res + p
            eres = _rounded(res, eres + ep)                # +
    return _based(res, eres, base)


def merged_values(e, weights, order=None, set_share=None, scale=1.0, base=None):
    return merged_rows(e, weights, order, set_share, scale, base)[0]
