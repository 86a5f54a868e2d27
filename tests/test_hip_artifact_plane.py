"""
GPU tests of the six consumers of svdq_merge.hip over the (k, r) plane (tests/artifact_plane.py): imported plans whose
every parameter sits at another (k, r) and another block / unit edge, against the fp64 model of the same artifacts.

  a. svdq_task_reconstruct (k_task_reconstruct): every element within the derived bound of ``task_values``
  b. svdq_merge (k_merge_reconstruct) at every compiled set count: within the bound of ``merged_values``
  c. the bit contracts the project states, over the plane: reconstruct_tasks == merge with the one-hot set ==
     reconstruct_from_coefficients (k_reconstruct, svdq_basis_ops.hip) on RTVQQuantizer.dequantize -- which puts k_reconstruct
     itself within the bound of fp64 at every (k, r)
  d. svdq_merge_masked / svdq_task_reconstruct_masked (k_merge_expand, k_task_expand): the bits of torch's boolean
     assignment of the plain route's compacted rows -- a block's first compacted row is anywhere, so both parts of a
     block start off a 16-byte boundary at every k
  e. svdq_diagnostics / svdq_diagnostics_masked (k_diag): helpers.diag_check on the artifacts the test made

The bound is artifact_plane's, derived there; nothing is skipped, and every input is finite by construction, so a
non-finite output fails.  Outputs are carved from one sentinel-filled buffer with 64-float gaps: whatever is not an
output still holds the sentinel afterwards.
"""
import numpy as np
import pytest
import torch

import artifact_plane as ap

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5C3E1      # a NaN no arithmetic here produces
GAP = 64
DENS = [0.9, 0.5, 0.97, 0.15, 0.3]

# name -> (N, fp16, center, stages)
CONFIGS = {}
for _n in ap.TASKS:
    for _fp16 in (True, False):
        for _center in (True, False):
            CONFIGS[f"n{_n}-{'fp16' if _fp16 else 'fp32'}-{'center' if _center else 'nocenter'}"] = (
                _n, _fp16, _center, ap.STAGES)
for _fp16 in (True, False):
    for _s in (1, 4):
        CONFIGS[f"n8-{'fp16' if _fp16 else 'fp32'}-stages{_s}"] = (8, _fp16, True, _s)
MASKED = {f"n{n}-{'fp16' if fp16 else 'fp32'}": (n, fp16) for n in ap.TASKS for fp16 in (True, False)}


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _import(c, plan_rows, dev):
    """An imported plan of the contents ``c`` declared at ``plan_rows``; returns (plan, U_high, U_low, mean on the device)."""
    from svdq_amd.pipeline import CompressPlan, pack_small
    plan = CompressPlan(plan_rows, c.n, center=c.center, fp16=c.fp16, low_bits=c.bits, rtvq_stages=c.stages, device=dev,
                        unit_rows=ap.UNIT_ROWS, workspace=False)
    host = pack_small(plan.layout, len(c.entries), c.n, c.stages, c.small_entries())
    uh = [None if e is None else e.U[:, :e.k].contiguous().to(dev) for e in c.entries]
    ul = [None if e is None else e.U[:, e.k:].contiguous().to(dev) for e in c.entries]
    mn = [None if e is None else e.mean.to(dev) for e in c.entries] if c.center else None
    plan.import_artifacts(uh, ul, mn, host)
    return plan, uh, ul, mn


def _sets(n, S, P, seed):
    """Multi-task sets with non-uniform weights renormalised per set, one task absent from set 0, a permuted order and a
    softmax share: ([S, N], [N], [S]) and the per-parameter forms ([P, S, N], [P, N], [P, S]) whose rows differ."""
    g = np.random.default_rng(seed)

    def one():
        w = np.full((S, n), -1.0, dtype=np.float32)
        for t in range(n):
            w[t % S, t] = 0.5 + g.random()
        w[0] = np.where(w[0] < 0, (0.25 + g.random(n)).astype(np.float32), w[0])      # set 0 holds every task ...
        if n > S:
            w[0, int(g.integers(S, n))] = -1.0                                         # ... but one
        for s in range(S):
            live = w[s] >= 0
            w[s, live] = (w[s, live] / w[s, live].sum(dtype=np.float32)).astype(np.float32)
        z = g.standard_normal(S)
        return w, g.permutation(n).astype(np.int32), (np.exp(z) / np.exp(z).sum()).astype(np.float32)
    w, o, sh = one()
    per = [one() for _ in range(P)]
    return (w, o, sh), tuple(np.stack([x[i] for x in per]) for i in range(3))


class _Case:
    """One imported plan of the plane, its base tensors and scales."""

    def __init__(self, key):
        n, fp16, center, stages = CONFIGS[key]
        self.dev = dev = torch.device("cuda", 0)
        self.c = c = ap.Contents(n, fp16=fp16, center=center, stages=stages)
        self.n, self.P = n, len(c.entries)
        self.plan, self.uh, self.ul, self.mn = _import(c, c.plan_rows, dev)
        self.rows, self.room = c.rows, c.plan_rows
        self.rows_dev = torch.tensor(c.rows, dtype=torch.int64).to(dev)
        g = torch.Generator().manual_seed(n + 17)
        self.base = [torch.randn(r, generator=g) for r in self.room]
        self.base_dev = [b.to(dev) for b in self.base]
        self.base_table = torch.tensor([b.data_ptr() for b in self.base_dev], dtype=torch.int64).to(dev)
        self.scale = np.array([(1.0, 0.3, 1.7)[p % 3] for p in range(self.P)], dtype=np.float32)
        self.scale_dev = torch.from_numpy(self.scale).to(dev)
        self._plain = None

    def tables(self, tabled):
        """rows_dev always: the parameter without rows exists through it (without it the declared rows hold)."""
        return dict(scale=self.scale_dev, base_table=self.base_table, rows_dev=self.rows_dev) if tabled else \
            dict(rows_dev=self.rows_dev)

    def plain(self):
        """reconstruct_tasks of all N tasks, no scale, no base: (host float32 buffer, device int32 buffer, offsets);
        computed once, left unchanged."""
        if self._plain is None:
            buf, offs, tab = _carve(self.room, self.n)
            self.plan.reconstruct_tasks(list(range(self.n)), tab, **self.tables(False))
            torch.cuda.synchronize()
            self._plain = (_host(buf), buf, offs)
        return self._plain


_CASES = {}


def _case(key):
    if key not in _CASES:
        _CASES[key] = _Case(key)
    return _CASES[key]


def _carve(room, n_out, skip=()):
    """One sentinel-filled buffer with an output of room[p] floats per (parameter, slot), GAP floats in front of, between
    and behind them.  Returns (buffer as int32, {(p, j): offset}, device table [P, n_out]); pairs in ``skip`` keep their
    room (the canary) but get a NULL table entry."""
    offs, pos = {}, GAP
    for p, r in enumerate(room):
        for j in range(n_out):
            offs[(p, j)] = pos
            pos += r + GAP
    buf = torch.full((pos,), SENTINEL, dtype=torch.int32, device="cuda")
    tab = np.zeros((len(room), n_out), dtype=np.int64)
    for (p, j), o in offs.items():
        if (p, j) not in skip:
            tab[p, j] = buf.data_ptr() + 4 * o
    return buf, offs, torch.from_numpy(tab).cuda()


def _host(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _untouched(host, offs, written):
    """Everything outside the written rows -- ``written(p, j)``: a row count or a bool array over the room -- still holds
    the sentinel."""
    outside = np.ones(host.size, dtype=bool)
    for (p, j), o in offs.items():
        w = written(p, j)
        if isinstance(w, (int, np.integer)):
            outside[o:o + int(w)] = False
        elif w is not None:
            outside[o:o + w.size] = ~w
    assert (host[outside].view(np.uint32) == SENTINEL).all(), "a write outside the outputs"


def _within(host, o, want, bound, what):
    """rows of the output at offset o against the model: finite and inside the bound, element by element."""
    got = host[o:o + want.size].view(np.float32)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - want)
    if not (err <= bound).all():
        i = int(np.argmax(err / bound))
        raise AssertionError((what, "row", i, "error / bound", float(err[i] / bound[i]), float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------ a. per-task reconstruction
@pytest.mark.parametrize("key", list(CONFIGS))
def test_reconstruct_tasks_within_the_bound_of_fp64(key):
    cs = _case(key)
    c = cs.c
    # the import put the contents where the consumers read them
    for p, e in c.live()[::7]:
        Uh, Ul, mean = cs.plan.basis_tensors(p, e.k, e.r, e.rows)
        assert torch.equal(Uh.cpu(), e.U[:, :e.k]) and torch.equal(Ul.cpu(), e.U[:, e.k:])
        assert mean is None or torch.equal(mean.cpu().reshape(-1), e.mean)
    for tabled in (False, True):
        if tabled:
            buf, offs, tab = _carve(cs.room, cs.n)
            cs.plan.reconstruct_tasks(list(range(cs.n)), tab, **cs.tables(True))
            host = _host(buf)
        else:
            host, _, offs = cs.plain()
        for p, e in c.live():
            want, bound = ap.task_rows(e, cs.scale[p], cs.base[p].numpy()) if tabled else ap.task_rows(e)
            for t in range(cs.n):
                _within(host, offs[(p, t)], want[:, t], bound[:, t], (key, tabled, p, t, e.rows, e.k, e.r))
        _untouched(host, offs, lambda p, j: cs.rows[p])


# ------------------------------------------------------------------------------------------ b. merge
@pytest.mark.parametrize("key", list(CONFIGS))
def test_merge_within_the_bound_of_fp64_at_every_set_count(key):
    cs = _case(key)
    c, dev = cs.c, cs.dev
    for S in (1, 2, 4, 8):
        if S > cs.n:
            continue
        (w, o, sh), (wp, op, shp) = _sets(cs.n, S, cs.P, 100 * cs.n + S)
        # one [S, N] table for all parameters, no scale, no base (one set: no share table)
        buf, offs, tab = _carve(cs.room, 1)
        share = None if S == 1 else sh
        cs.plan.merge(torch.from_numpy(w).to(dev), order=torch.from_numpy(o).to(dev),
                      set_share=None if share is None else torch.from_numpy(share).to(dev), out_table=tab,
                      **cs.tables(False))
        host = _host(buf)
        for p, e in c.live():
            want, bound = ap.merged_rows(e, w, o, share)
            _within(host, offs[(p, 0)], want, bound, (key, S, "[S, N]", p, e.rows, e.k, e.r))
        _untouched(host, offs, lambda p, j: cs.rows[p])
        # a [P, S, N] table whose rows differ per parameter, scale + base + rows_dev
        buf, offs, tab = _carve(cs.room, 1)
        cs.plan.merge(torch.from_numpy(wp).to(dev), order=torch.from_numpy(op).to(dev),
                      set_share=torch.from_numpy(shp).to(dev), out_table=tab, **cs.tables(True))
        host = _host(buf)
        for p, e in c.live():
            want, bound = ap.merged_rows(e, wp[p], op[p], shp[p], cs.scale[p], cs.base[p].numpy())
            _within(host, offs[(p, 0)], want, bound, (key, S, "[P, S, N]", p, e.rows, e.k, e.r))
        _untouched(host, offs, lambda p, j: cs.rows[p])


# ------------------------------------------------------------------------------------------ c. the bit contracts
@pytest.mark.parametrize("key", list(CONFIGS))
def test_one_hot_merges_and_the_per_parameter_route_give_the_same_bits(sq, key):
    cs = _case(key)
    c, dev = cs.c, cs.dev
    host, dbuf, offs = cs.plain()
    # merge with the one-hot set {j: 1.0}, written into a buffer carved the same way: the two buffers are equal as bits
    buf, offs2, tab = _carve(cs.room, cs.n)
    assert offs2 == offs
    for j in range(cs.n):
        w = torch.full((1, cs.n), -1.0)
        w[0, j] = 1.0
        cs.plan.merge(w.to(dev), out_table=tab[:, j].contiguous(), **cs.tables(False))
    torch.cuda.synchronize()
    if not torch.equal(buf, dbuf):
        other = _host(buf)
        for (p, j), o in offs.items():
            e = c.entries[p]
            assert np.array_equal(host[o:o + cs.rows[p]], other[o:o + cs.rows[p]]), (key, p, j, e.rows, e.k, e.r)
        raise AssertionError("the buffers differ outside the outputs")
    # the per-parameter route on the same U, c_high and the quantizer's own dequantized c_low
    quant = sq.RTVQQuantizer(c.bits, c.stages)
    for p, e in c.live():
        for t in sorted({0, cs.n - 1}):
            art = e.task_dict(t)
            cl = quant.dequantize(art["c_low_quant"], device="cuda") if e.r > e.k else torch.zeros(0, device=dev)
            assert np.array_equal(cl.cpu().numpy().view(np.uint32), ap.coef(e, t)[e.k:].view(np.uint32)), (key, p, t)
            uh = cs.uh[p] if e.k else torch.empty((e.rows, 0), dtype=e.U.dtype, device=dev)
            ul = cs.ul[p] if e.r > e.k else torch.empty((e.rows, 0), dtype=e.U.dtype, device=dev)
            got = sq.reconstruct_from_coefficients(art["c_high_fp16"], cl, uh, ul, device="cuda",
                                                   mean=None if cs.mn is None else cs.mn[p])
            o = offs[(p, t)]
            assert got.dtype is torch.float32 and got.shape == (e.rows,)
            assert np.array_equal(got.cpu().numpy().view(np.int32), host[o:o + e.rows]), (key, p, t, e.rows, e.k, e.r)


# ------------------------------------------------------------------------------------------ d. the masked forms
class _Masked:
    """A centred plan of the plane declared at source sizes: parameter p's rows are the selected (odd p: the cleared)
    elements of a mask that selects exactly rows[p] of ceil(rows[p] / density) positions."""

    def __init__(self, key):
        from svdq_amd.mask_loader import MaskSet
        n, fp16 = MASKED[key]
        self.dev = dev = torch.device("cuda", 0)
        self.c = c = ap.Contents(n, fp16=fp16, center=True, zero=False, seed=1)
        self.n, self.P, self.rows = n, len(c.entries), c.rows
        g = torch.Generator().manual_seed(900 + n)
        self.sizes = [int(np.ceil(r / DENS[p % len(DENS)])) for p, r in enumerate(c.rows)]
        self.inv = [p % 2 == 1 for p in range(self.P)]
        self.sel, masks = [], []
        for p, (r, D) in enumerate(zip(c.rows, self.sizes)):
            s = torch.zeros(D, dtype=torch.bool)
            s[torch.randperm(D, generator=g)[:r]] = True
            self.sel.append(s)
            masks.append(~s if self.inv[p] else s)
        self.plan, self.uh, self.ul, self.mn = _import(c, self.sizes, dev)
        self.ms = MaskSet(self.sizes, dev)
        ct, cf = self.ms.count_scan([m.to(dev) for m in masks])
        self.rows_dev = torch.where(torch.tensor(self.inv, device=dev), cf, ct)
        assert self.rows_dev.tolist() == c.rows
        self.mtab = torch.tensor([m.data_ptr() for m in self.ms._s["mb"]], dtype=torch.int64).to(dev)
        self.us = self.ms.unit_starts(self.plan, self.rows_dev, entry_map=[(q, self.inv[q]) for q in range(self.P)])
        self.base = [torch.randn(D, generator=g) for D in self.sizes]
        self.base_dev = [b.to(dev) for b in self.base]
        self.btab = torch.tensor([b.data_ptr() for b in self.base_dev], dtype=torch.int64).to(dev)
        self.fill1 = torch.ones(self.P, dtype=torch.int32, device=dev)
        self.sel_np = [s.numpy() for s in self.sel]
        # the plain route's compacted rows of every task: computed once, left unchanged
        buf, self.coffs, tab = _carve(c.rows, n)
        self.plan.reconstruct_tasks(list(range(n)), tab, rows_dev=self.rows_dev)
        self.compact = _host(buf)

    def expanded(self, p, rows_bits, fill=True, base=True):
        """torch's boolean assignment of compacted rows (int32 bits of float32), + base: the bits of the full output;
        without fill the rows that are not selected keep the sentinel."""
        z = torch.zeros(self.sizes[p])
        z[self.sel[p]] = torch.from_numpy(rows_bits.view(np.float32).copy())
        full = (self.base[p] + z) if base else z
        out = full.numpy().view(np.int32).copy()
        if not fill:
            out[~self.sel_np[p]] = np.uint32(SENTINEL).astype(np.int32)
        return out


_MASKED = {}


def _masked(key):
    if key not in _MASKED:
        _MASKED[key] = _Masked(key)
    return _MASKED[key]


@pytest.mark.parametrize("key", list(MASKED))
def test_masked_task_reconstruction_is_the_plain_route_put_back(key):
    m = _masked(key)
    c, n = m.c, m.n
    # the plain route on this plan too sits inside the bound of fp64
    for p, e in c.live():
        want, bound = ap.task_rows(e)
        for t in range(n):
            _within(m.compact, m.coffs[(p, t)], want[:, t], bound[:, t], (key, "compact", p, t, e.rows, e.k, e.r))
    _untouched(m.compact, m.coffs, lambda p, j: m.rows[p])

    def compact(p, t):
        o = m.coffs[(p, t)]
        return m.compact[o:o + m.rows[p]]
    pick = sorted({0, n - 1, n // 2}) + [n // 2]      # a permuted subset with a duplicate
    pick = pick[::-1]
    for tasks, fill, skip in ((list(range(n)), True, set()), (list(range(n)), False, set()),
                              (pick, True, {(p, j) for p in range(m.P) for j in range(len(pick)) if (p + 2 * j) % 5 == 0})):
        buf, offs, tab = _carve(m.sizes, len(tasks), skip)
        m.plan.reconstruct_tasks_masked(tasks, m.mtab, m.us, m.rows_dev, tab, fill=m.fill1 if fill else None,
                                        base_table=m.btab)
        host = _host(buf)
        for (p, j), o in offs.items():
            e = c.entries[p]
            want = np.full(m.sizes[p], np.uint32(SENTINEL).astype(np.int32)) if (p, j) in skip else \
                m.expanded(p, compact(p, tasks[j]), fill)
            assert np.array_equal(host[o:o + m.sizes[p]], want), (key, fill, p, j, tasks[j], e.rows, e.k, e.r)
        _untouched(host, offs, lambda p, j: None if (p, j) in skip else (m.sizes[p] if fill else m.sel_np[p]))


@pytest.mark.parametrize("key", list(MASKED))
def test_masked_merge_is_the_plain_merge_put_back(key):
    m = _masked(key)
    c, n, dev = m.c, m.n, m.dev
    for S in (1, 2, 4, 8):
        if S > n:
            continue
        (w, o, sh), _ = _sets(n, S, m.P, 300 * n + S)
        fill = S in (1, 4)
        args = dict(order=torch.from_numpy(o).to(dev), set_share=None if S == 1 else torch.from_numpy(sh).to(dev))
        cbuf, coffs, ctab = _carve(m.rows, 1)
        m.plan.merge(torch.from_numpy(w).to(dev), rows_dev=m.rows_dev, out_table=ctab, **args)
        buf, offs, tab = _carve(m.sizes, 1)
        m.plan.merge_masked(torch.from_numpy(w).to(dev), m.mtab, m.us, m.rows_dev, tab, fill=m.fill1 if fill else None,
                            base_table=m.btab, **args)
        chost, host = _host(cbuf), _host(buf)
        for p, e in c.live():
            want, bound = ap.merged_rows(e, w, o, None if S == 1 else sh)
            _within(chost, coffs[(p, 0)], want, bound, (key, S, "compact", p, e.rows, e.k, e.r))
            rows = chost[coffs[(p, 0)]:coffs[(p, 0)] + e.rows]
            got = host[offs[(p, 0)]:offs[(p, 0)] + m.sizes[p]]
            assert np.array_equal(got, m.expanded(p, rows, fill)), (key, S, fill, p, e.rows, e.k, e.r)
        _untouched(chost, coffs, lambda p, j: m.rows[p])
        _untouched(host, offs, lambda p, j: m.sizes[p] if fill else m.sel_np[p])


# ------------------------------------------------------------------------------------------ e. diagnostics
def _deltas(c, seed):
    """x[p][t] float32 CPU: the task's own values + noise of a tenth of the typical magnitude + one spike per task at a
    block-boundary row."""
    g = torch.Generator().manual_seed(seed)
    xs = []
    for p, e in enumerate(c.entries):
        if e is None:
            xs.append([torch.zeros(c.plan_rows[p]) for _ in range(c.n)])
            continue
        typ = 1.0 / np.sqrt(e.rows)
        vals = ap.task_rows(e)[0]
        spots = [s for s in (0, 63, 64, 127, 128, 255, 256, 4095, 4096, 8191, 8192, e.rows - 2, e.rows - 1) if 0 <= s < e.rows]
        row = []
        for t in range(c.n):
            x = torch.from_numpy(vals[:, t]).float() + 0.1 * typ * torch.randn(e.rows, generator=g)
            x[spots[(t + p) % len(spots)]] += (3.0 + 0.25 * t) * typ
            row.append(x)
        xs.append(row)
    return xs


def _check_diag(c, res, xs, what, add_mean=False):
    from helpers import diag_check
    from oracle import svd_hybrid_oracle as orc
    assert np.isfinite(np.stack([res[p] for p, _ in c.live()])).all(), what
    for p, e in c.live():
        Uh, Ul = e.U[:, :e.k], e.U[:, e.k:]
        for t in range(c.n):
            cf = torch.from_numpy(ap.coef(e, t))
            diag_check(dict(zip(orc.DIAG_KEYS, res[p, t])), xs[p][t], Uh, Ul, cf[:e.k], cf[e.k:],
                       what=(what, p, t, e.rows, e.k, e.r), mean=e.mean.reshape(-1, 1) if add_mean else None)


@pytest.mark.parametrize("key", list(CONFIGS))
def test_diagnostics_against_fp64_on_the_artifacts(key):
    cs = _case(key)
    c = cs.c
    xs = _deltas(c, 77 + cs.n)
    table = cs.plan.pointer_table([[x.to(cs.dev) for x in row] for row in xs])
    res = cs.plan.diagnostics(table, rows_dev=cs.rows_dev).cpu().numpy()
    _check_diag(c, res, xs, key)
    if c.center:
        res = cs.plan.diagnostics(table, rows_dev=cs.rows_dev, add_mean=True).cpu().numpy()
        _check_diag(c, res, xs, (key, "add_mean"), add_mean=True)


@pytest.mark.parametrize("key", list(MASKED))
def test_masked_diagnostics_against_fp64_on_the_artifacts(key):
    m = _masked(key)
    c = m.c
    xs = _deltas(c, 78 + m.n)
    g = torch.Generator().manual_seed(5)
    full = []
    for p, row in enumerate(xs):
        typ = 1.0 / np.sqrt(m.rows[p])
        fs = []
        for x in row:
            f = torch.randn(m.sizes[p], generator=g) * typ      # what the mask leaves out is not the task's
            f[m.sel[p]] = x
            fs.append(f.to(m.dev))
        full.append(fs)
    table = m.plan.pointer_table(full)
    res = m.plan.diagnostics_masked(table, m.mtab, m.us, m.rows_dev).cpu().numpy()
    _check_diag(c, res, xs, (key, "walk"))
    res = m.plan.diagnostics_masked(table, m.mtab, m.us, m.rows_dev, add_mean=True).cpu().numpy()
    _check_diag(c, res, xs, (key, "walk", "add_mean"), add_mean=True)
