"""
GPU tests of svdq_plan_residual_gram / svdq_plan_extend_basis (include/svdq.h; CompressPlan.residual_gram /
extend_basis): the stored basis of a plan grown by the directions new tasks add outside its span.

Every plan is filled with svdq_plan_import from tensors the test makes itself, so k, r and the basis are free.  The
fp64 model of the three steps (residual, residual Gram, eigen stage) is written in numpy below and works from the bytes
the kernels read: the stored U as float, ``coef`` from the small buffer, xc formed with the same fp32 subtractions.

Bounds (u = 2^-24), all derived, none measured:
  e      the kernel's e is xc followed by r fmas: at most r + 1 roundings of partial results that never exceed
         |xc| + sum |U||c| in magnitude, so |e_hat - e| <= (r + 2) u (|xc| + sum_i |U_i||c_i|) =: de, per element.
  H      H_hat = fl(sum e_hat_i e_hat_j): the data error sum (|e_i| de_j + |e_j| de_i + de_i de_j), plus the
         accumulation -- an fp32 chain over at most 256 rows, fp64 beyond: 258 u sum |e_hat_i e_hat_j| as in
         test_hip_plan_project.py.  n_j: 258 u sum xc^2 (xc itself is exact).
  lambda Weyl: |lambda_hat_i - lambda_i| <= |dH|_2 <= |dH|_F =: h.
  w      Davis-Kahan: sin(theta_i) <= h / (gap_i - h), gap_i the distance of lambda_i to the rest of the spectrum; with
         h <= gap_i / 4 (asserted) the sign-aligned unit eigenvectors differ by at most sqrt(2) sin(theta) <= 2 h / gap_i.
  d      d = sqrt(lambda) w: |dd| <= h / sqrt(lambda_i) + sqrt(lambda_i) 2 h / gap_i + u |d| (the fp32 store).
  Q      q_i = E z_i, z_i = w_i / sqrt(lambda_i): |dz_i|_2 <= 2 h / (gap_i sqrt(lambda_i)) + h / lambda_i^1.5, so per
         element |dq| <= sum_j de_j |z_ji| + |e[d, :]|_2 |dz_i|_2 + (M + 2) u sum_j |e_j||z_ji| (the fma chain over the
         slots and the fp32 store of Z) + u_Q |q| (the store in the basis type).
The fixtures are conditioned (asserted from the model, so a regenerated fixture cannot drift): on every kept direction
lambda_max / lambda_i <= 100, consecutive lambdas differ by >= 2 x, |xc_j| / |e_j| <= 4.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
MINRES = 2.0 ** -12
SENT = 0x5A
GUARD = 64
UNIT_ROWS = 256
# rows of the basis (None: a parameter whose rows are 0) and the kind of (k, r) it stores
# with the block edges of both block sizes (256 rows up to 16 slots, 128 above): 1, RB - 1, RB, RB + 1, 2 RB + 1
SHAPES = [(1, "k=r"), (13, "r<N"), (255, "k0"), (256, "k=r<N"), (257, "r<N"), (None, "k0"), (700, "r=N"),
          (127, "r<N"), (128, "k=r<N"), (129, "k0"), (513, "r=N")]
ABSENT_P = 3      # the last new task lacks this parameter
CASES = [(n, m) for n in (8, 9, 17) for m in (1, 3, 8)]


def _kr(rows, n, kind):
    if kind == "k=r":
        r = min(rows, n)
        return r, r
    if kind == "k0":
        return 0, min(rows, n)
    if kind == "k=r<N":
        r = min(rows, n - 1)
        return r, r
    if kind == "r=N":
        return 1, min(rows, n)
    r = min(rows, max(1, min(4, n // 2)))      # r < N
    return r // 2, r


def _orthonormal(rows, cols, g):
    q, _ = torch.linalg.qr(torch.randn(rows, cols, generator=g, dtype=torch.float64))
    return q


class Fixture:
    """A ragged plan with stored (rounded, nearly orthonormal) bases and M new tasks whose residual spectrum is set:
    lambda_i = 2.1^-i over min(present, 7, D - r) directions.  Eight spaced lambdas would span 2^7 > 100, so with eight
    present tasks the last is a bitwise copy of the first (and the mixing matrix W has those two rows equal, its columns
    still orthonormal): H then has two identical rows and an eighth eigenvalue at fp64 round-off.  A direction that is
    only NEARLY dependent would not do: the fp32 chain of a block leaves H_hat off by ~1e-6 lambda_max, above the
    threshold min_residual^2 = 6e-8 relative to max |xc|^2, so such a lambda_hat may land on either side of it."""

    def __init__(self, n, M, *, fp16, center, shapes=SHAPES, absent=((ABSENT_P, -1),), input_dtype=torch.float32,
                 seed=0, random_basis=False):
        from svdq_amd.pipeline import CompressPlan, pack_small
        dev = torch.device("cuda", 0)
        g = torch.Generator().manual_seed(100 * n + M + 7 * seed)
        self.n, self.M, self.fp16, self.center, self.dev = n, M, fp16, center, dev
        self.rows = [r if r is not None else 0 for r, _ in shapes]
        self.plan_rows = [r if r is not None else 300 for r, _ in shapes]
        self.plan = CompressPlan(self.plan_rows, n, center=center, fp16=fp16, low_bits=4, rtvq_stages=2, device=dev,
                                 unit_rows=UNIT_ROWS, input_dtype=input_dtype, workspace=False)
        udt = torch.float16 if fp16 else torch.float32
        self.udt = udt
        self.absent = {(p, t % M) for p, t in absent}
        self.kr, self.U, self.mean, self.x, entries = [], [], [], [], []
        for p, (rows, kind) in enumerate(shapes):
            if rows is None:
                self.kr.append((0, 0))
                self.U.append(None)
                self.mean.append(None)
                self.x.append([torch.zeros(1) for _ in range(M)])
                entries.append(None)
                continue
            k, r = _kr(rows, n, kind)
            basis = _orthonormal(rows, rows if rows < r + 8 else r + 8, g)
            uf = basis[:, :r]
            if random_basis:
                uf = torch.randn(rows, r, generator=g, dtype=torch.float64) / np.sqrt(rows)
            u = uf.to(udt)
            mean = (torch.randn(rows, generator=g) * 0.01) if center else None
            present = [t for t in range(M) if (p, t) not in self.absent]
            nd = max(0, min(len(present), 7, rows - r))
            xs = [None] * M
            if present:
                W = _orthonormal(len(present), len(present), g)
                twin = len(present) == 8
                if twin:      # rows 0 and 7 equal, columns orthonormal: 2 (v0 / sqrt 2)(v0 / sqrt 2)^T + sum v_j v_j^T = I
                    V = _orthonormal(7, 7, g)
                    W = torch.cat([V[:1] / np.sqrt(2.0), V[1:], V[:1] / np.sqrt(2.0)])
                s = torch.tensor([2.1 ** (-0.5 * i) for i in range(nd)], dtype=torch.float64)
                E = basis[:, r:r + nd] @ torch.diag(s) @ W[:, :nd].T if nd else torch.zeros(rows, len(present),
                                                                                           dtype=torch.float64)
                for a, t in enumerate(present):
                    en = float(E[:, a].norm())
                    coef = torch.randn(r, generator=g, dtype=torch.float64)
                    coef = coef / max(float(coef.norm()), 1e-30) * max(0.5 * en, 0.1) if r else coef
                    xt = E[:, a] + u.double() @ coef
                    if mean is not None:
                        xt = xt + mean.double()
                    xs[t] = xt.float()
                if twin:
                    xs[present[7]] = xs[present[0]].clone()
            self.kr.append((k, r))
            self.U.append(u)
            self.mean.append(mean)
            self.x.append(xs)
            entries.append({"rows": rows, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
                            "c_high": np.zeros((n, k), np.float16), "codes": np.zeros((n, 2, r - k), np.uint8),
                            "scale": np.zeros((n, 2), np.float32), "zero_point": np.zeros((n, 2), np.float32),
                            "residual_norm": np.zeros((n, 2), np.float32)})
        host = pack_small(self.plan.layout, len(shapes), n, 2, entries)
        uh = [None if u is None else u[:, :k].contiguous().to(dev) for u, (k, r) in zip(self.U, self.kr)]
        ul = [None if u is None else u[:, k:].contiguous().to(dev) for u, (k, r) in zip(self.U, self.kr)]
        mn = [None if m is None else m.to(dev) for m in self.mean] if center else None
        self.plan.import_artifacts(uh, ul, mn, host)
        self.rows_dev = torch.tensor(self.rows, dtype=torch.int64).to(dev)
        self._keep = []

    # ---- tables
    def table(self, tensors):
        """tensors[p][t] for t < M (None = absent) -> the int64 [P * N] device table; slots >= M are absent."""
        self._keep.append(tensors)
        flat = []
        for ts in tensors:
            flat += [0 if t is None else t.data_ptr() for t in ts] + [0] * (self.n - len(ts))
        return torch.tensor(flat, dtype=torch.int64).to(self.dev)

    def ptrs(self, tensors):
        self._keep.append(tensors)
        return torch.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch.int64).to(self.dev)

    def cuda_inputs(self, xs=None):
        xs = self.x if xs is None else xs
        return [[None if x is None else x.cuda() for x in row] for row in xs]

    # ---- the three steps on the GPU
    def run(self, table=None, min_residual=MINRES, write=True, **args):
        """project -> residual Gram -> (read m) -> write.  Returns a dict of host copies."""
        pl = self.plan
        table = self.table(self.cuda_inputs()) if table is None else table
        args.setdefault("rows_dev", self.rows_dev)
        sm = pl.project_tasks(table, **args)
        ext = pl.residual_gram(table, self.M, min_residual=min_residual, **args)
        n_units = int(pl.sizes.n_units)
        per = [-(-r // UNIT_ROWS) for r in self.plan_rows]
        assert sum(per) == n_units          # the unit order this file reads the partials in
        part = pl._extend_work[:n_units * 64 * 8].view(torch.float64).cpu().numpy().reshape(n_units, 8, 8)
        H, u0 = [], 0
        for c in per:
            H.append(part[u0:u0 + c].sum(axis=0))
            u0 += c
        # the work buffer's two arrays (the alignment gap between them and the tail are never written)
        wb = pl._extend_work.cpu().numpy()
        n_off = -(-n_units * 512 // 256) * 256
        res = {"sm": sm, "ext": ext, "H": H, "ext_bytes": pl.extension.cpu().numpy().copy(),
               "work_bytes": np.concatenate([wb[:n_units * 512], wb[n_off:n_off + n_units * 64]]), "out": None,
               "bufs": None}
        if write:
            outs, bufs = [], []
            es = 2 if self.fp16 else 4
            for p, rows in enumerate(self.rows):
                m = int(ext.m[p])
                k = self.kr[p][0]
                if m == 0 or rows == 0:
                    outs.append(None)
                    bufs.append(None)
                    continue
                nel = rows * (k + m)
                buf = torch.full(((2 * GUARD + nel) * es,), SENT, dtype=torch.uint8, device=self.dev)
                bufs.append(buf)
                outs.append(buf[GUARD * es:(GUARD + nel) * es].view(self.udt).view(rows, k + m))
            pl.extend_basis(table, self.M, outs, **args)
            torch.cuda.synchronize()
            res["out"] = [None if o is None else o.cpu() for o in outs]
            res["bufs"] = [None if b is None else b.cpu().numpy() for b in bufs]
        return res

    # ---- the fp64 model of one entry, from the bytes the kernels read
    def model(self, p, coef, min_residual=MINRES, xs=None):
        rows = self.rows[p]
        k, r = self.kr[p]
        xs = self.x[p] if xs is None else xs
        present = [t for t in range(self.M) if xs[t] is not None]
        Uf = self.U[p].double().numpy()
        Xc = np.zeros((rows, self.M))
        for t in present:
            xc = xs[t].float()
            if self.mean[p] is not None:
                xc = xc - self.mean[p]          # one fp32 subtraction
            Xc[:, t] = xc.double().numpy()
        C = np.zeros((r, self.M))
        for t in present:
            C[:, t] = coef[p, t, :r].astype(np.float64)
        E = Xc - Uf @ C
        de = (r + 2) * U32 * (np.abs(Xc) + np.abs(Uf) @ np.abs(C))
        H = E.T @ E
        aE = np.abs(E)
        dH = aE.T @ de + de.T @ aE + de.T @ de + 258 * U32 * ((aE + de).T @ (aE + de))
        nrm = (Xc ** 2).sum(axis=0)
        h = float(np.linalg.norm(dH))
        out = {"present": present, "Xc": Xc, "C": C, "E": E, "de": de, "H": H, "dH": dH, "n": nrm, "h": h, "Uf": Uf}
        if not present:
            out.update(m=0, lam=np.zeros(0), W=np.zeros((0, 0)))
            return out
        Hp = H[np.ix_(present, present)]
        lam, W = np.linalg.eigh(Hp)
        lam, W = lam[::-1].copy(), W[:, ::-1].copy()
        for i in range(len(present)):
            j = int(np.argmax(np.abs(W[:, i])))
            if W[j, i] < 0:
                W[:, i] = -W[:, i]
        thr = min_residual ** 2 * nrm[present].max()
        cap = min(len(present), rows - r)
        m = 0
        while m < cap and lam[m] > thr:
            m += 1
        out.update(m=m, lam=lam, W=W, thr=thr)
        return out


def _conditioned(md):
    """The fixture conditions of the module docstring, from the model; returns gap_i of the kept directions."""
    m, lam, present = md["m"], md["lam"], md["present"]
    gaps = []
    for i in range(m):
        assert lam[0] / lam[i] <= 100.0, (i, lam)
        if i + 1 < len(lam):
            assert lam[i] >= 2.0 * max(lam[i + 1], 0.0), (i, lam)
        others = np.delete(lam, i)
        gaps.append(float(np.min(np.abs(others - lam[i]))) if len(others) else float("inf"))
        assert md["h"] <= gaps[-1] / 4
    if m:
        for t in present:
            xn, en = np.sqrt(md["n"][t]), np.sqrt(md["H"][t, t])
            assert xn <= 4.0 * en, (t, xn, en)
    return gaps


_cache = {}


def _case(n, M, fp16, center):
    key = (n, M, fp16, center)
    if key not in _cache:
        fx = Fixture(n, M, fp16=fp16, center=center)
        _cache[key] = (fx, fx.run())
    return _cache[key]


PARAMS = [pytest.param(n, M, fp16, center, id=f"n{n}-M{M}-{'fp16' if fp16 else 'fp32'}-{'c' if center else 'nc'}")
          for n, M in CASES for fp16 in (True, False) for center in (True, False)]


# ------------------------------------------------------------------------------------------ 1. H and n_j
@pytest.mark.parametrize("n,M,fp16,center", PARAMS)
def test_gram_and_norms_against_the_model(n, M, fp16, center):
    fx, res = _case(n, M, fp16, center)
    ext = res["ext"]
    for p, rows in enumerate(fx.rows):
        if rows == 0:
            assert not res["H"][p].any() and int(ext.m[p]) == 0
            continue
        md = fx.model(p, res["sm"].coef)
        Hk = res["H"][p]
        err = np.abs(Hk[:M, :M] - md["H"])
        print(p, "H err / bound", float((err / np.maximum(md["dH"], 1e-300)).max()))
        assert (err <= md["dH"]).all(), (p, float((err / np.maximum(md["dH"], 1e-300)).max()))
        assert not Hk[M:].any() and not Hk[:, M:].any()
        absent = [t for t in range(M) if t not in md["present"]]
        assert not Hk[absent].any() and not Hk[:, absent].any()
        assert (np.abs(ext.xnorm[p, :M] - md["n"]) <= 258 * U32 * md["n"]).all()
        assert np.array_equal(ext.enorm[p, :M], np.diag(Hk)[:M])
        assert not ext.xnorm[p, M:].any() and not ext.enorm[p, M:].any()


# ------------------------------------------------------------------------------------------ 2. m, lambda, d, Q
@pytest.mark.parametrize("n,M,fp16,center", PARAMS)
def test_eigen_stage_and_new_columns_against_the_model(n, M, fp16, center):
    fx, res = _case(n, M, fp16, center)
    ext = res["ext"]
    uq = 2.0 ** -11 if fp16 else U32
    seen = 0
    for p, rows in enumerate(fx.rows):
        if rows == 0:
            continue
        k, r = fx.kr[p]
        md = fx.model(p, res["sm"].coef)
        gaps = _conditioned(md)
        m, lam, W, present, h = md["m"], md["lam"], md["W"], md["present"], md["h"]
        assert int(ext.m[p]) == m, (p, int(ext.m[p]), m, lam)
        assert m == max(0, min(len(present), 7, rows - r))      # what the fixture was built to give
        assert (np.abs(ext.lam[p, :len(present)] - lam) <= h + 1e-13 * lam[0]).all() if present else True
        assert not ext.z[p, :, m:].any() and not ext.d[p, :, m:].any()
        if m == 0:
            assert res["out"][p] is None
            continue
        seen += m
        Q = res["out"][p].double().numpy()[:, k:]
        E, de = md["E"], md["de"]
        for i in range(m):
            w, sl = W[:, i], np.sqrt(lam[i])
            dw = 2 * h / gaps[i]
            dgot = ext.d[p, present, i].astype(np.float64)
            dref = sl * w
            # the sign rule decides by the largest component: where the two largest are closer than the eigenvector
            # bound the other sign is as right
            top = np.sort(np.abs(w))[::-1]
            flip = len(top) > 1 and top[0] - top[1] <= 2 * dw and np.abs(dgot + dref).max() < np.abs(dgot - dref).max()
            sg = -1.0 if flip else 1.0
            bd = h / sl + sl * dw + U32 * np.abs(dref) + 1e-13 * np.sqrt(lam[0])
            assert (np.abs(dgot - sg * dref) <= bd).all(), (p, i, np.abs(dgot - sg * dref) / bd)
            z = np.zeros(fx.M)
            z[present] = sg * w / sl
            dz = dw / sl + h / lam[i] ** 1.5
            qref = E @ z
            bq = (de @ np.abs(z) + np.linalg.norm(E, axis=1) * dz + (M + 2) * U32 * (np.abs(E) @ np.abs(z))
                  + uq * np.abs(qref) + 1e-30)
            errq = np.abs(Q[:, i] - qref)
            assert (errq <= bq).all(), (p, i, float((errq / bq).max()))
        # orthonormality.  Before the store, Q^T Q = Z^T H Z with Z from H_hat: I - Z^T dH Z, and |z_i^T dH z_j| <=
        # h / sqrt(l_i l_j); the chain over the slots (and the fp32 store of Z) moves q_i elementwise by at most
        # (M + 2) u |E||z_i|, so Q^T Q by at most 2 (M + 2) u s_i s_j with s_i = | |E||z_i| |_2 >= |q_i|_2.  The store in
        # the basis type rounds q elementwise, q~ = q (1 + delta), |delta| <= u_Q: by Cauchy-Schwarz it moves q_i . q_j
        # by at most (2 u_Q + u_Q^2) |q_i|_2 |q_j|_2, in terms of the stored columns (2 u_Q + 3 u_Q^2) |q~_i|_2 |q~_j|_2
        # -- the COLUMN NORMS, which are 1 to within this very bound, not s_i.  (An fp16 element below 2^-14 is rounded to
        # 2^-25 absolutely instead: at most 2^-24 sqrt(D) over a column pair.)
        # In the issue's form, 2 u_Q + c u sqrt(l_max / l_i) |xc| / |e| with rho = max |xc_j| / |e_j| (<= 4) and
        # l_max / l_i <= 100:  the data part of dH gives z_i^T E^T dE z_j <= |dE|_F / sqrt(l_j) with |dE|_F <=
        # (r + 2)(1 + sqrt(r)) u sqrt(M) rho sqrt(l_max), twice; the accumulation part 258 u M l_max / sqrt(l_i l_j)
        # <= 2580 u M sqrt(l_max / l_i) rho; the chain 2 (M + 2) M u l_max / sqrt(l_i l_j) likewise.  So
        # c = 2 (r + 2)(1 + sqrt(r)) sqrt(M) + 2580 M + 20 (M + 2) M.  The second-order terms of the store (3 u_Q^2,
        # 2 u_Q (|q~_i||q~_j| - 1), the subnormal 2^-24 sqrt(D): below 3e-6 in all at D <= 700) are below the 2580 M u >=
        # 1.5e-4 of the accumulation part, whose worst case a 256-row chain does not come near.
        G = Q.T @ Q - np.eye(m)
        S = np.array([np.linalg.norm(np.abs(E[:, present]) @ np.abs(W[:, i] / np.sqrt(lam[i]))) for i in range(m)])
        nq = np.linalg.norm(Q, axis=0)
        lamk = lam[:m]
        store = (2 * uq + 3 * uq * uq) * np.outer(nq, nq) + (2.0 ** -24 * np.sqrt(rows) if fp16 else 0.0)
        fine = store + h / np.sqrt(np.outer(lamk, lamk)) + 2 * (M + 2) * U32 * np.outer(S, S)
        print(p, "|Q^T Q - I| max", float(np.abs(G).max()), "of the fine bound", float((np.abs(G) / fine).max()))
        assert (np.abs(G) <= fine).all(), (p, float((np.abs(G) / fine).max()))
        rho = max(np.sqrt(md["n"][t] / md["H"][t, t]) for t in present)
        c = 2 * (r + 2) * (1 + np.sqrt(r)) * np.sqrt(M) + 2580 * M + 20 * (M + 2) * M
        coarse = 2 * uq + c * U32 * np.sqrt(lam[0] / lamk)[None, :] * rho
        assert (np.abs(G) <= coarse).all(), (p, float((np.abs(G) / coarse).max()))
    assert seen > 0


# ------------------------------------------------------------------------------------------ 3. what users get
@pytest.mark.parametrize("n,M,fp16,center", PARAMS)
def test_new_tasks_are_reconstructed_to_the_threshold(n, M, fp16, center):
    """|xc_j - U c_j - Q d_j|_2 <= u_Q | |Q||d_j| |_2 + fp32 terms + min_residual sqrt(M) max |xc|.  Q d_j = E W W^T
    delta_j for whatever orthonormal W the eigen stage found, so the eigenvector error does not enter: the fp32 terms
    are |de_j|_2 + |de|_F (e_hat for e, on both sides), (M + 4) u | |E||Z||d_j| |_2 (the chain over the slots, Z and d
    stored as fp32), and sqrt(h) where directions were dropped (their lambda_hat is below the threshold, lambda within
    h of it).  Without the new columns the same quantity is |e_j|: at least 10 x larger here."""
    fx, res = _case(n, M, fp16, center)
    ext = res["ext"]
    uq = 2.0 ** -11 if fp16 else U32
    checked = 0
    for p, rows in enumerate(fx.rows):
        if rows == 0 or int(ext.m[p]) == 0:
            continue
        k, r = fx.kr[p]
        md = fx.model(p, res["sm"].coef)
        m, present = int(ext.m[p]), md["present"]
        Q = res["out"][p].double().numpy()[:, k:]
        xmax = np.sqrt(md["n"][present].max())
        Z = ext.z[p, :M, :m].astype(np.float64)
        for t in present:
            d = ext.d[p, t, :m].astype(np.float64)
            e = md["E"][:, t]
            got = np.linalg.norm(e - Q @ d)
            fp32 = (np.linalg.norm(md["de"][:, t]) + np.linalg.norm(md["de"])
                    + (M + 4) * U32 * np.linalg.norm(np.abs(md["E"]) @ np.abs(Z) @ np.abs(d))
                    + (np.sqrt(md["h"]) if m < len(present) else 0.0))
            bound = uq * np.linalg.norm(np.abs(Q) @ np.abs(d)) + fp32 + MINRES * np.sqrt(M) * xmax
            print(p, t, "residual", got, "bound", bound, "without the new columns", np.linalg.norm(e))
            assert got <= bound, (p, t, got, bound)
            assert np.linalg.norm(e) >= 10 * got, (p, t)
            checked += 1
    assert checked > 0


# ------------------------------------------------------------------------------------------ 4. nothing old moves
@pytest.mark.parametrize("n,M,fp16,center", PARAMS[::5])
def test_stored_columns_and_plan_buffers_are_only_read(n, M, fp16, center):
    fx = Fixture(n, M, fp16=fp16, center=center)
    pl = fx.plan
    table = fx.table(fx.cuda_inputs())
    pl.project_tasks(table, rows_dev=fx.rows_dev)
    before = (pl.basis.cpu().numpy().copy(), None if pl.mean is None else pl.mean.cpu().numpy().copy(),
              pl.small.cpu().numpy().copy())
    res = fx.run(table=table)
    assert np.array_equal(pl.basis.cpu().numpy(), before[0])
    assert pl.mean is None or np.array_equal(pl.mean.cpu().numpy(), before[1])
    assert np.array_equal(pl.small.cpu().numpy(), before[2])      # project_tasks ran twice on the same inputs
    for p, out in enumerate(res["out"]):
        if out is None:
            continue
        k = fx.kr[p][0]
        assert out[:, :k].numpy().tobytes() == fx.U[p][:, :k].numpy().tobytes()


# ------------------------------------------------------------------------------------------ 5. null and edge cases
def _one(rows, n, M, *, kind, fp16=False, center=False, random_basis=False):
    return Fixture(n, M, fp16=fp16, center=center, shapes=[(rows, kind)], absent=(), random_basis=random_basis)


def test_task_in_the_span_adds_nothing_and_changes_nothing():
    """mean + U a: m = 0, no output, and the small buffer is what project_tasks alone leaves."""
    fx = _one(700, 8, 2, kind="r<N", fp16=True, center=True)
    g = torch.Generator().manual_seed(3)
    u, mean = fx.U[0].double(), fx.mean[0].double()
    fx.x[0] = [(mean + u @ torch.randn(fx.kr[0][1], generator=g, dtype=torch.float64)).float() for _ in range(2)]
    table = fx.table(fx.cuda_inputs())
    fx.plan.project_tasks(table, rows_dev=fx.rows_dev)
    plain = fx.plan.small.cpu().numpy().copy()
    res = fx.run(table=table)
    assert int(res["ext"].m[0]) == 0 and res["out"][0] is None
    assert np.array_equal(fx.plan.small.cpu().numpy(), plain)
    assert not res["ext"].z.any() and not res["ext"].d.any()


def test_two_identical_tasks_add_one_column():
    fx = _one(257, 8, 2, kind="r<N", fp16=False, center=False)
    fx.x[0][1] = fx.x[0][0].clone()
    res = fx.run()
    assert int(res["ext"].m[0]) == 1
    lam = res["ext"].lam[0]
    assert lam[0] > 0 and abs(lam[1]) <= 1e-6 * lam[0]
    assert np.allclose(res["ext"].d[0, 0, 0], res["ext"].d[0, 1, 0], rtol=1e-6)


def test_m_is_capped_by_the_rows_left():
    """D = 1 (r = 1: no room) and D - r < M with a basis that is not orthonormal, so that the residuals have full rank."""
    fx = _one(1, 8, 3, kind="k=r")
    assert int(fx.run()["ext"].m[0]) == 0
    fx = _one(13, 8, 8, kind="k0", random_basis=True)      # r = 8: five rows left
    g = torch.Generator().manual_seed(11)
    fx.x[0] = [torch.randn(13, generator=g) for _ in range(8)]
    res = fx.run()
    md = fx.model(0, res["sm"].coef)
    assert md["lam"][5] > md["thr"]          # the threshold alone would keep more
    assert int(res["ext"].m[0]) == 5 and res["out"][0].shape == (13, 5)


def test_all_zero_task_on_an_uncentred_plan_adds_nothing():
    fx = _one(300, 9, 1, kind="r<N", fp16=True, center=False)
    fx.x[0] = [torch.zeros(300)]
    res = fx.run()
    assert int(res["ext"].m[0]) == 0 and not res["ext"].xnorm.any() and not res["ext"].lam.any()


@pytest.mark.parametrize("n", [8, 17])
def test_spikes_land_in_their_rows(n):
    """One large element on a zero background at the first and last row of a block, a unit and the parameter, k = r = 0
    rows kept out of it by a basis that is zero there: e = xc, H is diagonal, and Q has +-1 exactly at the spike."""
    rows = 700
    blk = 256 if n <= 16 else 128
    spikes = [0, blk - 1, blk, UNIT_ROWS - 1, UNIT_ROWS, 2 * UNIT_ROWS - 1, 2 * UNIT_ROWS, rows - 1]
    spikes = sorted(set(spikes))      # six rows at n = 8, eight at n = 17: the parameter's last row is always one
    M = len(spikes)
    assert spikes[-1] == rows - 1 and M <= 8
    fx = _one(rows, n, M, kind="r<N", fp16=False, center=False)
    for s in spikes:
        fx.U[0][s] = 0
    k, r = fx.kr[0]
    # the plan was imported in the constructor: import the edited basis again
    from svdq_amd.pipeline import pack_small
    entry = {"rows": rows, "k": k, "r": r, "energy": 0.5, "sigma": np.ones(r, np.float32),
             "c_high": np.zeros((n, k), np.float16), "codes": np.zeros((n, 2, r - k), np.uint8),
             "scale": np.zeros((n, 2), np.float32), "zero_point": np.zeros((n, 2), np.float32),
             "residual_norm": np.zeros((n, 2), np.float32)}
    fx.plan.import_artifacts([fx.U[0][:, :k].contiguous().cuda()], [fx.U[0][:, k:].contiguous().cuda()], None,
                             pack_small(fx.plan.layout, 1, n, 2, [entry]))
    fx.x[0] = [torch.zeros(rows) for _ in range(M)]
    for t, s in enumerate(spikes):
        fx.x[0][t][s] = float(2.0 ** (8 - t))        # lambda_t = 4^(8 - t): descending in slot order
    res = fx.run()
    assert int(res["ext"].m[0]) == M
    Q = res["out"][0][:, k:].double().numpy()
    want = np.zeros((rows, M))
    for t, s in enumerate(spikes):
        want[s, t] = 1.0
    assert np.array_equal(Q, want)
    assert np.array_equal(res["ext"].lam[0, :M], np.array([4.0 ** (8 - t) for t in range(M)]))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_input_is_flagged(bad):
    """A NaN or Inf in one new task: n_j of the entry is not finite in the extension buffer, nothing is decomposed
    (m = 0, zeros), the healthy entries are what they are without it, and CompressPlan.residual_gram raises."""
    from svdq_amd.pipeline import NonFiniteInput, extend_views
    want = Fixture(8, 3, fp16=True, center=True).run(write=False)["ext"]
    fx = Fixture(8, 3, fp16=True, center=True)
    p = 4                                    # 257 rows
    fx.x[p][1][200] = bad
    table = fx.table(fx.cuda_inputs())
    fx.plan.project_tasks(table, rows_dev=fx.rows_dev)
    with pytest.raises(NonFiniteInput) as exc:
        fx.plan.residual_gram(table, 3, rows_dev=fx.rows_dev)
    assert exc.value.indices == [p]
    ext = extend_views(fx.plan.extension.cpu().numpy(), fx.plan.extend_layout(), fx.plan.P)
    assert not np.isfinite(ext.xnorm[p, 1]) and np.isfinite(np.delete(ext.xnorm, p, axis=0)).all()
    assert int(ext.m[p]) == 0 and not ext.lam[p].any() and not ext.z[p].any() and not ext.d[p].any()
    for q in range(len(fx.rows)):
        if q != p:
            assert int(ext.m[q]) == int(want.m[q]) and np.array_equal(ext.lam[q], want.lam[q])
            assert np.array_equal(ext.z[q], want.z[q]) and np.array_equal(ext.d[q], want.d[q])


# ------------------------------------------------------------------------------------------ 6. input forms
def _three(res):
    return res["work_bytes"], res["ext_bytes"], [None if o is None else o.view(torch.uint8).numpy() for o in res["out"]]


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))


@pytest.mark.parametrize("n,M", [(8, 3), (17, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_from_base_and_half_inputs_are_the_plain_call_bit_for_bit(n, M, dtype):
    g = torch.Generator().manual_seed(5)
    ref = Fixture(n, M, fp16=True, center=True)
    base = [torch.randn(max(r, 1), generator=g).to(dtype) for r in ref.rows]
    ft = [[None if x is None else (base[p].float() + x).to(dtype) for x in row] for p, row in enumerate(ref.x)]
    delta = [[None if f is None else f.float() - base[p].float() for f in row] for p, row in enumerate(ft)]
    want = _three(ref.run(table=ref.table(ref.cuda_inputs(delta))))
    assert any(o is not None for o in want[2])
    fx = Fixture(n, M, fp16=True, center=True, input_dtype=dtype)
    got = _three(fx.run(table=fx.table(fx.cuda_inputs(ft)), base_table=fx.ptrs([b.cuda() for b in base])))
    _same(got, want)


@pytest.mark.parametrize("n,M", [(9, 3), (17, 8)])
def test_index_lists_are_the_plain_call_on_gathered_rows(n, M):
    g = torch.Generator().manual_seed(9)
    ref = Fixture(n, M, fp16=False, center=True)
    want = _three(ref.run())
    fx = Fixture(n, M, fp16=False, center=True)
    full, idx = [], []
    for p, rows in enumerate(fx.rows):
        numel = 2 * max(rows, 1) + 5
        sel = torch.sort(torch.randperm(numel, generator=g)[:max(rows, 1)]).values
        idx.append(sel.int().cuda())
        row = []
        for x in fx.x[p]:
            if x is None:
                row.append(None)
                continue
            big = torch.randn(numel, generator=g)
            big[sel[:x.numel()]] = x
            row.append(big)
        full.append(row)
    got = _three(fx.run(table=fx.table(fx.cuda_inputs(full)), index_table=fx.ptrs(idx)))
    _same(got, want)


# ------------------------------------------------------------------------------------------ 7. determinism, guards, refusals
@pytest.mark.parametrize("n,M,fp16,center", PARAMS[2::7])
def test_two_runs_give_the_same_bytes_and_nothing_is_written_outside(n, M, fp16, center):
    fx, res = _case(n, M, fp16, center)
    again = fx.run()
    _same(_three(again), _three(res))
    es = 2 if fp16 else 4
    wrote = 0
    for buf in res["bufs"]:
        if buf is None:
            continue
        assert (buf[:GUARD * es] == SENT).all() and (buf[-GUARD * es:] == SENT).all()
        wrote += 1
    assert wrote > 0


def test_refusals_come_before_any_launch():
    from svdq_amd import _native as nat
    fx = Fixture(8, 2, fp16=True, center=True)
    pl, lib = fx.plan, nat.lib()
    table = fx.table(fx.cuda_inputs())
    pl.project_tasks(table, rows_dev=fx.rows_dev)
    pl.residual_gram(table, 2, rows_dev=fx.rows_dev)
    ext_before = pl.extension.cpu().numpy().copy()
    work = pl._extend_work
    P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    good = [pl._h, P(table), None, None, P(fx.rows_dev), P(pl.basis), P(pl.mean), P(pl.small), 2, MINRES,
            P(pl.extension), P(work), None]

    def gram(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.svdq_plan_residual_gram(*a)

    assert gram() == nat.SVDQ_OK
    for bad in (dict(a1=None), dict(a5=None), dict(a7=None), dict(a10=None), dict(a11=None),      # NULLs
                dict(a6=None),                                                                      # centred, no mean
                dict(a1=P(table) + 4), dict(a11=P(work) + 4), dict(a10=P(pl.extension) + 8),        # misalignment
                dict(a7=P(pl.small) + 8), dict(a8=0), dict(a8=9), dict(a9=-1.0), dict(a9=float("nan"))):
        assert gram(**bad) == nat.SVDQ_EINVAL, bad
    otab = torch.zeros(pl.P, dtype=torch.int64, device=fx.dev)
    goodw = good[:9] + [P(pl.extension), P(otab), None]
    assert lib.svdq_plan_extend_basis(*goodw) == nat.SVDQ_OK            # every out NULL: nothing is written
    for i, v in ((1, None), (9, None), (10, None), (6, None), (10, P(otab) + 4), (8, 9), (8, 0)):
        a = list(goodw)
        a[i] = v
        assert lib.svdq_plan_extend_basis(*a) == nat.SVDQ_EINVAL, (i, v)
    with pytest.raises(ValueError):
        pl.residual_gram(table, 9, rows_dev=fx.rows_dev)
    torch.cuda.synchronize()
    assert np.array_equal(pl.extension.cpu().numpy(), ext_before)
