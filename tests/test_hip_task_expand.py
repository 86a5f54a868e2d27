"""
GPU tests of svdq_task_reconstruct_masked (include/svdq.h; CompressPlan.reconstruct_tasks_masked; k_task_expand): every
selected task's own reconstruction of the MASKED regions of a plan, written at the source rows inside one streaming
launch.  The contract is bits, twice over: an output is what svdq_merge_masked gives with that task as a one-hot set,
and what svdq_task_reconstruct gives in compacted rows once torch's boolean assignment has put them back (+ base).
Against the oracle's matmul the project's tolerance for that comparison holds.

Shapes: test_plan_merge_masked_at_every_block_size's ragged sizes and densities, plus one crafted parameter whose mask
has a run of 800 cleared rows (whole chunks that select nothing, at the 256-row and at the 128-row chunk size).  Task
counts on both sides of the 16-task chunk-size switch, of the 1 / 4 / 8 task groups and at the limit; both polarities.
Outputs are carved from one buffer pre-filled with a sentinel, 64-float gaps between them: whatever is not an output
row still holds the sentinel afterwards.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [9000, 300, 4096 * 3 + 5, 8192 + 300, 61, 1500]
DENS = [0.9, 0.5, 0.97, 0.15, 0.4, None]      # None: the crafted mask
SENTINEL = 0x7FA5C3E1      # a NaN no arithmetic here produces
GAP = 64

# name -> (N, fp16, inverted, center)
CONFIGS = {
    "n1-fp16": (1, True, False, True),
    "n3-fp32": (3, False, False, True),
    "n8-fp16": (8, True, False, True),
    "n12-fp32-inv": (12, False, True, True),
    "n20-fp16": (20, True, False, True),
    "n20-fp32-inv": (20, False, True, True),
    "n32-fp16": (32, True, False, True),
    "n8-fp16-nocenter": (8, True, False, False),
}
FINITE_CONFIG = "n8-fp16"
ORACLE_CONFIGS = ["n1-fp16", "n3-fp32", "n8-fp16", "n12-fp32-inv", "n20-fp16", "n32-fp16"]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _bits(a, b):
    """Bit-for-bit equality of two tensors (NaN equals the same NaN, -0.0 differs from +0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(w), b.to(a.device).contiguous().view(w))


def _masks(n_tasks):
    """The same masks for every configuration of one task count (a signal plan and a noise plan share them)."""
    gen = torch.Generator().manual_seed(200 + n_tasks)
    out = []
    for D, q in zip(SIZES, DENS):
        if q is not None:
            out.append(torch.rand(D, generator=gen) < q)
            continue
        m = torch.zeros(D, dtype=torch.bool)
        m[:300] = True                                        # 300..1099 stay clear
        m[1100:1499] = torch.rand(399, generator=gen) < 0.5
        m[1499] = True
        out.append(m)
    return out


class _Case:
    """One compressed plan of masked regions, its tables, and -- computed once, left unchanged -- the N one-hot
    svdq_merge_masked results (fill = 1, + base) and the N compacted-row reconstructions of svdq_task_reconstruct."""

    def __init__(self, key):
        from oracle import svd_hybrid_oracle as orc
        from svdq_amd.mask_loader import MaskSet
        from svdq_amd.pipeline import CompressPlan
        n, fp16, inverted, center = CONFIGS[key]
        dev = torch.device("cuda", 0)
        self.n, self.inverted = n, inverted
        vecs = [[d.to(dev) for d in orc.synthetic_deltas(D, n, 700 + i, rank=min(3, n))] for i, D in enumerate(SIZES)]
        self.masks = [m.to(dev) for m in _masks(n)]
        self.sel = [(~m if inverted else m) for m in self.masks]
        self.ms = MaskSet(SIZES, dev)
        ct, cf = self.ms.count_scan(self.masks)
        self.rows_dev = cf if inverted else ct
        self.plan = plan = CompressPlan(SIZES, n, energy_threshold=0.9, max_rank=None, center=center, fp16=fp16,
                                        low_bits=4, rtvq_stages=2, device=dev)
        P = len(SIZES)
        self.mtab = torch.tensor([c.data_ptr() for c in self.ms._s["mb"]], dtype=torch.int64).to(dev)
        self.us = self.ms.unit_starts(plan, self.rows_dev, entry_map=[(q, inverted) for q in range(P)])
        comp = [[torch.cat([v[s_], torch.zeros(D - int(s_.sum()), device=dev)]) for v in vs]
                for vs, s_, D in zip(vecs, self.sel, SIZES)]
        plan.run(plan.pointer_table(comp), self.rows_dev)
        self.small = plan.fetch_small()
        self.rows = [int(r) for r in self.small.rows[:P]]
        assert self.rows == [int(s_.sum()) for s_ in self.sel]
        g = torch.Generator().manual_seed(n)
        self.base = [torch.randn(D, generator=g).to(dev) for D in SIZES]
        self.btab = torch.tensor([b.data_ptr() for b in self.base], dtype=torch.int64).to(dev)
        self.fill1 = torch.ones(P, dtype=torch.int32, device=dev)
        # (b) the one-hot merges, full tensors, fill = 1, + base
        self.want = []      # [task][param]
        for t in range(n):
            w = torch.full((1, n), -1.0)
            w[0, t] = 1.0
            full = [torch.full((D,), float("nan"), device=dev) for D in SIZES]
            otab = torch.tensor([f.data_ptr() for f in full], dtype=torch.int64).to(dev)
            plan.merge_masked(w.to(dev), self.mtab, self.us, self.rows_dev, otab, fill=self.fill1, base_table=self.btab)
            self.want.append(full)
        # (a) the compacted rows of svdq_task_reconstruct (no base, no scale)
        offs, tot = [], 0
        for p in range(P):
            for t in range(n):
                offs.append(tot)
                tot += (self.rows[p] + 63) // 64 * 64
        cbuf = torch.zeros(max(tot, 1), dtype=torch.float32, device=dev)
        ctab = torch.tensor([cbuf.data_ptr() + 4 * o for o in offs], dtype=torch.int64).to(dev)
        plan.reconstruct_tasks(list(range(n)), ctab, rows_dev=self.rows_dev)
        self.compact = [[cbuf[offs[p * n + t]:offs[p * n + t] + self.rows[p]] for p in range(P)] for t in range(n)]
        torch.cuda.synchronize()

    def call(self, pick, tab, fill=True, base=True, scale=None):
        self.plan.reconstruct_tasks_masked(pick, self.mtab, self.us, self.rows_dev, tab, scale=scale,
                                           fill=self.fill1 if fill else None, base_table=self.btab if base else None)


_CASES = {}


def _case(key):
    if key not in _CASES:
        _CASES[key] = _Case(key)
    return _CASES[key]


def _carve(n_out, skip=()):
    """One sentinel-filled buffer with a FULL output of SIZES[p] floats per (parameter, slot), GAP floats in front of,
    between and behind them.  Returns (buffer as int32, {(p, j): offset}, device table [P, n_out]); pairs in ``skip``
    keep their room (the canary) but get a NULL table entry."""
    offs, pos = {}, GAP
    for p, D in enumerate(SIZES):
        for j in range(n_out):
            offs[(p, j)] = pos
            pos += D + GAP
    buf = torch.full((pos,), SENTINEL, dtype=torch.int32, device="cuda")
    tab = np.zeros((len(SIZES), n_out), dtype=np.int64)
    for (p, j), o in offs.items():
        if (p, j) not in skip:
            tab[p, j] = buf.data_ptr() + 4 * o
    return buf, offs, torch.from_numpy(tab).cuda()


def _check(buf, offs, want_of, skip=(), written_of=None):
    """Every output row that is to be written holds the wanted bits; everything else -- gaps, skipped outputs and, with
    ``written_of`` (p -> bool rows), the rows an output leaves alone -- still the sentinel."""
    torch.cuda.synchronize()
    outside = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for (p, j), o in offs.items():
        if (p, j) in skip:
            continue
        got = buf[o:o + SIZES[p]].view(torch.float32)
        want = want_of(p, j)
        if written_of is None:
            assert _bits(got, want), (p, j, SIZES[p])
            outside[o:o + SIZES[p]] = False
        else:
            wr = written_of(p)
            assert _bits(got[wr], want[wr]), (p, j, SIZES[p])
            outside[o:o + SIZES[p]] = ~wr
    assert bool((buf[outside] == SENTINEL).all()), "a write outside the rows of the outputs"


# ------------------------------------------------------------------------------------------ the contract on bits
@pytest.mark.parametrize("key", list(CONFIGS))
def test_all_tasks_in_one_call_are_the_one_hot_masked_merges(key):
    c = _case(key)
    buf, offs, tab = _carve(c.n)
    c.call(list(range(c.n)), tab)
    # (b) svdq_merge_masked with the one-hot set
    _check(buf, offs, lambda p, j: c.want[j][p])
    # (a) svdq_task_reconstruct in compacted rows, torch's boolean assignment, + base
    for p, D in enumerate(SIZES):
        for t in range(c.n):
            z = torch.zeros(D, device="cuda")
            z[c.sel[p]] = c.compact[t][p]
            o = offs[(p, t)]
            assert _bits(buf[o:o + D].view(torch.float32), c.base[p] + z), (p, t)


@pytest.mark.parametrize("key", ["n8-fp16", "n20-fp32-inv"])
def test_without_fill_the_unselected_rows_are_left_alone(key):
    c = _case(key)
    buf, offs, tab = _carve(c.n)
    c.call(list(range(c.n)), tab, fill=False)
    _check(buf, offs, lambda p, j: c.want[j][p], written_of=lambda p: c.sel[p])
    # and without a base table the value alone is written
    buf, offs, tab = _carve(c.n)
    c.call(list(range(c.n)), tab, fill=True, base=False)

    def plain(p, j):
        z = torch.zeros(SIZES[p], device="cuda")
        z[c.sel[p]] = c.compact[j][p]
        return z
    _check(buf, offs, plain)


def test_signal_and_noise_plans_write_the_same_tensors(sq):
    """reconstruct_from_masked (mask_loader.py:712-763): result[mask] = signal rows, result[~mask] = noise rows -- the
    signal plan and the inverted noise plan (scale = 0.5), neither filling, between them write every row once."""
    from svdq_amd.mask_loader import reconstruct_from_masked
    sig, noi = _case("n20-fp16"), _case("n20-fp32-inv")
    assert all(torch.equal(a, b) for a, b in zip(sig.masks, noi.masks))
    n = sig.n
    half = torch.full((len(SIZES),), 0.5, dtype=torch.float32, device="cuda")
    buf, offs, tab = _carve(n)
    sig.call(list(range(n)), tab, fill=False, base=False)
    noi.call(list(range(n)), tab, fill=False, base=False, scale=half)
    # the noise rows in compacted form, with the same scale
    o2, tot = [], 0
    for p in range(len(SIZES)):
        for t in range(n):
            o2.append(tot)
            tot += (noi.rows[p] + 63) // 64 * 64
    nbuf = torch.zeros(tot, dtype=torch.float32, device="cuda")
    ntab = torch.tensor([nbuf.data_ptr() + 4 * o for o in o2], dtype=torch.int64).cuda()
    noi.plan.reconstruct_tasks(list(range(n)), ntab, scale=half, rows_dev=noi.rows_dev)
    torch.cuda.synchronize()

    def want(p, j):
        nrows = nbuf[o2[p * n + j]:o2[p * n + j] + noi.rows[p]]
        return reconstruct_from_masked(sig.compact[j][p], nrows, sig.masks[p], torch.Size([SIZES[p]]))
    _check(buf, offs, want)


# ------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("key,pick", [("n8-fp16", [5, 2, 7, 2]),                                # one group of four
                                      ("n20-fp16", [16, 0, 9, 9, 3, 12, 1, 19, 8, 4]),          # two groups of eight
                                      ("n12-fp32-inv", [11, 0, 3, 3, 7, 1, 9, 10, 2])])
def test_permuted_subset_duplicates_null_outputs_and_a_device_table(key, pick):
    c = _case(key)
    P = len(SIZES)
    skip = {(p, j) for p in range(P) for j in range(len(pick)) if (p + 2 * j) % 5 == 0}
    skip |= {(3, j) for j in range(len(pick))}                                  # a parameter nobody wants
    buf, offs, tab = _carve(len(pick), skip)
    c.call(pick, tab)
    _check(buf, offs, lambda p, j: c.want[pick[j]][p], skip)
    # the same selection as an int32 device table; an index outside [0, N) there is skipped like a NULL output
    dev_pick = torch.tensor(pick[:-1] + [c.n], dtype=torch.int32).cuda()
    last = {(p, len(pick) - 1) for p in range(P)}
    buf, offs, tab = _carve(len(pick))
    c.call(dev_pick, tab)
    _check(buf, offs, lambda p, j: c.want[pick[j]][p], last)


# ------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_refused_before_anything_is_launched(sq):
    from ctypes import c_void_p
    nat = sq._native
    c = _case("n8-fp16")
    plan, lib = c.plan, nat.lib()
    buf, offs, tab = _carve(c.n)
    idx = torch.arange(c.n, dtype=torch.int32).cuda()
    work = torch.empty(int(lib.svdq_task_reconstruct_work_bytes(plan._h, c.n)), dtype=torch.uint8, device="cuda")
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(task=c_void_p(idx.data_ptr()), n_out=c.n, masks=c_void_p(c.mtab.data_ptr()),
                starts=c_void_p(c.us.data_ptr()), out=c_void_p(tab.data_ptr()), mean=c_void_p(plan.mean.data_ptr()))

    def call(**over):
        a = dict(good, **over)
        return lib.svdq_task_reconstruct_masked(plan._h, c_void_p(c.rows_dev.data_ptr()), c_void_p(plan.small.data_ptr()),
                                                c_void_p(plan.basis.data_ptr()), a["mean"], a["task"], a["n_out"], None,
                                                a["masks"], a["starts"], c_void_p(c.fill1.data_ptr()),
                                                c_void_p(c.btab.data_ptr()), a["out"], c_void_p(work.data_ptr()), stream)
    for n_out in (0, 33, -1):
        assert call(n_out=n_out) == nat.SVDQ_EINVAL
        assert "n_out" in nat.last_error()
    for name in ("task", "out", "masks", "starts", "mean"):      # mean: the plan is centred
        assert call(**{name: None}) == nat.SVDQ_EINVAL, name
        assert "svdq_task_reconstruct_masked" in nat.last_error()
    # indices are checked where the host sees them: the call that builds the device table
    for bad in ([0, c.n], [-1], [], list(range(33))):
        with pytest.raises(ValueError, match="svdq_task_reconstruct"):
            c.call(bad, tab)
    with pytest.raises(ValueError, match="out_table"):
        c.call([0, 1], tab)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert call() == nat.SVDQ_OK      # the same call, well-formed
    _check(buf, offs, lambda p, j: c.want[j][p])


# ------------------------------------------------------------------------------------------ graph capture
def test_capture_and_replay_give_the_eager_bits():
    c = _case("n20-fp16")
    pick = list(range(c.n))
    buf, offs, tab = _carve(c.n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.call(pick, tab)      # warm-up outside the capture: work buffer, task table
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = buf.clone()
    buf.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c.call(pick, tab)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())      # capture does not execute
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager)
    _check(buf, offs, lambda p, j: c.want[j][p])


# ------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("key", ORACLE_CONFIGS)
def test_against_the_oracle_on_the_fetched_artifacts(key):
    """orc.reconstruct (a matmul) on the plan's own basis, fp16 c_high and oracle-dequantized c_low, put back with
    torch's boolean assignment: the tolerance of tests/test_hip_task_reconstruct.py."""
    from oracle import svd_hybrid_oracle as orc
    c = _case(key)
    sm = c.small
    buf, offs, tab = _carve(c.n)
    c.call(list(range(c.n)), tab, base=False)
    torch.cuda.synchronize()
    host = buf.cpu().view(torch.float32).numpy()
    finite = True
    for p, D in enumerate(SIZES):
        k, r, rows = int(sm.k[p]), int(sm.r[p]), c.rows[p]
        Uh, Ul, mean = (None if x is None else x.cpu() for x in c.plan.basis_tensors(p, k, r, rows))
        sel = c.sel[p].cpu().numpy()
        for t in range(c.n):
            ch = torch.from_numpy(sm.c_high[p, t, :k].astype(np.float32))
            cl = torch.from_numpy(orc.rtvq_dequantize({"codes": sm.codes[p, t, :, :r - k], "scale": sm.scale[p, t],
                                                       "zero_point": sm.zero_point[p, t]}).astype(np.float32).reshape(-1))
            want = np.zeros(D, dtype=np.float32)
            want[sel] = orc.reconstruct(ch, cl, Uh, Ul, mean).numpy().reshape(-1)
            o = offs[(p, t)]
            np.testing.assert_allclose(host[o:o + D], want, rtol=1e-5, atol=1e-6, err_msg=f"{p} {t}")
            finite = finite and bool(np.isfinite(want).all())
    # equality is not trivial: on a configuration whose rows are finite (a rank-deficient synthetic set is not, and is
    # compared like any other) something is non-zero and two tasks differ
    if key == FINITE_CONFIG:
        assert finite
        o0, o1 = offs[(0, 0)], offs[(0, 1)]
        assert float(np.abs(host[o0:o0 + SIZES[0]]).max()) > 0
        assert not np.array_equal(host[o0:o0 + SIZES[0]], host[o1:o1 + SIZES[0]])
