"""
GPU tests of svdq_task_reconstruct (include/svdq.h; CompressPlan.reconstruct_tasks): every selected task's own
reconstruction of every parameter of a plan from ONE pass over the basis.  The contract is bits: a (parameter, task)
output is what svdq_merge gives with that task as a one-hot set (and so what svdq_reconstruct gives on that task's
coefficients).  Against the oracle's matmul the project's tolerance for that comparison holds, so the two kernels cannot
share a mistake unseen.

Shapes: tests/test_hip_adopt.py's -- one ragged parameter set per configuration, the smallest rows at which a block, a
unit or a tail can go wrong; task counts on both sides of the 16-task block-size switch, of the 8-task group and at
the limit.  Outputs are carved from one buffer pre-filled with a sentinel, 64-float gaps between them: whatever is
not an output still holds the sentinel afterwards.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 13, 255, 256, 257, 4095, 4096, 4097, 8193, 70001]
TASK_COUNTS = [1, 3, 8, 17, 32]
SENTINEL = 0x7FA5C3E1      # a NaN no arithmetic here produces
GAP = 64

# name -> (N, fp16, center, energy_threshold, max_rank)
CONFIGS = {}
for _n in TASK_COUNTS:
    for _fp16 in (True, False):
        for _center in (True, False):
            CONFIGS[f"n{_n}-{'fp16' if _fp16 else 'fp32'}-{'center' if _center else 'nocenter'}"] = (
                _n, _fp16, _center, 0.9, None)
CONFIGS["energy1"] = (8, True, True, 1.0, None)      # k = r: U_low is empty
CONFIGS["energy1-nocenter"] = (8, True, False, 1.0, None)
CONFIGS["maxrank1"] = (8, True, True, 0.9, 1)
ORACLE_CONFIGS = [f"n{n}-fp16-center" for n in TASK_COUNTS]
FINITE_CONFIGS = ORACLE_CONFIGS + ["energy1-nocenter", "maxrank1"]


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


class _Case:
    """One compressed plan, its tables, and -- computed once, left unchanged -- the N one-hot merges of the plan,
    plain and with scale + base."""

    def __init__(self, key):
        from oracle import svd_hybrid_oracle as orc
        from svdq_amd.pipeline import compress_batch
        n, fp16, center, energy, max_rank = CONFIGS[key]
        self.n = n
        vecs = [[d.cuda() for d in orc.synthetic_deltas(rows, n, 31 * n + rows, rank=min(3, n))] for rows in ROWS]
        self.plan, self.small = compress_batch(vecs, energy_threshold=energy, max_rank=max_rank, center=center, fp16=fp16,
                                               low_bits=4, rtvq_stages=2, device="cuda")
        P = len(ROWS)
        g = torch.Generator().manual_seed(n)
        self.base = [torch.randn(rows, generator=g).cuda() for rows in ROWS]
        self.base_table = torch.tensor([b.data_ptr() for b in self.base], dtype=torch.int64).cuda()
        self.scale = torch.tensor([0.5 if p % 2 else 1.0 for p in range(P)], dtype=torch.float32).cuda()
        self.want = {False: [], True: []}      # [tabled][task][param]
        for tabled in (False, True):
            for t in range(n):
                w = torch.full((1, n), -1.0)
                w[0, t] = 1.0
                buf, offs, tab = self.plan.new_merged_outputs()
                self.plan.merge(w.cuda(), out_table=tab, **self.tables(tabled))
                self.want[tabled].append([buf[offs[p]:offs[p] + rows] for p, rows in enumerate(ROWS)])
        torch.cuda.synchronize()

    def tables(self, tabled):
        return dict(scale=self.scale, base_table=self.base_table) if tabled else {}


_CASES = {}


def _case(key):
    if key not in _CASES:
        _CASES[key] = _Case(key)
    return _CASES[key]


def _carve(n_out, skip=()):
    """One sentinel-filled buffer with an output of rows[p] floats per (parameter, slot), GAP floats in front of, between
    and behind them.  Returns (buffer as int32, {(p, j): offset}, device table [P, n_out]); pairs in ``skip`` keep their
    room (the canary) but get a NULL table entry."""
    offs, pos = {}, GAP
    for p, rows in enumerate(ROWS):
        for j in range(n_out):
            offs[(p, j)] = pos
            pos += rows + GAP
    buf = torch.full((pos,), SENTINEL, dtype=torch.int32, device="cuda")
    tab = np.zeros((len(ROWS), n_out), dtype=np.int64)
    for (p, j), o in offs.items():
        if (p, j) not in skip:
            tab[p, j] = buf.data_ptr() + 4 * o
    return buf, offs, torch.from_numpy(tab).cuda()


def _check(buf, offs, want_of, skip=()):
    """Every output holds the wanted bits; everything else -- gaps, tails, skipped outputs -- still the sentinel."""
    torch.cuda.synchronize()
    outside = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for (p, j), o in offs.items():
        if (p, j) in skip:
            continue
        got = buf[o:o + ROWS[p]].view(torch.float32)
        assert _bits(got, want_of(p, j)), (p, j, ROWS[p])
        outside[o:o + ROWS[p]] = False
    assert bool((buf[outside] == SENTINEL).all()), "a write outside the outputs"


# ------------------------------------------------------------------------------------------ plan level
@pytest.mark.parametrize("key", list(CONFIGS))
def test_all_tasks_in_one_call_are_the_one_hot_merges(key):
    c = _case(key)
    for tabled in (False, True):
        buf, offs, tab = _carve(c.n)
        c.plan.reconstruct_tasks(list(range(c.n)), tab, **c.tables(tabled))
        _check(buf, offs, lambda p, j: c.want[tabled][j][p])
    # the outputs are not trivially equal: finite, two tasks differ somewhere, nothing is all zero.  (Checked where the
    # merge's own rows are finite; at "energy1" and "n3-fp32-nocenter" they are not, and are compared as bits like any
    # others -- "energy1-nocenter" is the empty-U_low case with finite rows.)
    if key in FINITE_CONFIGS:
        last = [w[-1] for w in c.want[False]]
        assert all(bool(torch.isfinite(w).all()) for w in last) and float(last[0].abs().max()) > 0
        assert c.n == 1 or not _bits(last[0], last[1])


@pytest.mark.parametrize("key", ORACLE_CONFIGS)
def test_against_the_oracle_on_the_fetched_artifacts(key):
    """orc.reconstruct (a matmul) on the plan's own basis, fp16 c_high and oracle-dequantized c_low: the tolerance of
    test_reconstruct_kernel_vs_oracle."""
    from oracle import svd_hybrid_oracle as orc
    c = _case(key)
    sm = c.small
    buf, offs, tab = _carve(c.n)
    c.plan.reconstruct_tasks(list(range(c.n)), tab)
    torch.cuda.synchronize()
    host = buf.cpu().view(torch.float32).numpy()
    for p, rows in enumerate(ROWS):
        k, r = int(sm.k[p]), int(sm.r[p])
        Uh, Ul, mean = (None if x is None else x.cpu() for x in c.plan.basis_tensors(p, k, r, rows))
        for t in range(c.n):
            ch = torch.from_numpy(sm.c_high[p, t, :k].astype(np.float32))
            cl = torch.from_numpy(orc.rtvq_dequantize({"codes": sm.codes[p, t, :, :r - k], "scale": sm.scale[p, t],
                                                       "zero_point": sm.zero_point[p, t]}).astype(np.float32).reshape(-1))
            want = orc.reconstruct(ch, cl, Uh, Ul, mean).numpy()
            o = offs[(p, t)]
            np.testing.assert_allclose(host[o:o + rows], want, rtol=1e-5, atol=1e-6, err_msg=f"{p} {t}")


# ------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("key", ["n8-fp16-center", "n17-fp32-nocenter"])
def test_permuted_subset_duplicates_and_null_outputs(key):
    c = _case(key)
    pick = [5, 2, 7, 2] if c.n == 8 else [16, 0, 9, 9, 3, 12, 1, 15, 8, 4]      # ten slots: two groups of 8
    skip = {(p, j) for p in range(len(ROWS)) for j in range(len(pick)) if (p + 2 * j) % 5 == 0}
    skip |= {(3, j) for j in range(len(pick))}                                  # a parameter nobody wants
    for tabled in (False, True):
        buf, offs, tab = _carve(len(pick), skip)
        c.plan.reconstruct_tasks(pick, tab, **c.tables(tabled))
        _check(buf, offs, lambda p, j: c.want[tabled][pick[j]][p], skip)
    # the same selection as an int32 device table; an index outside [0, N) there is skipped like a NULL output
    dev_pick = torch.tensor(pick[:-1] + [c.n], dtype=torch.int32).cuda()
    last = {(p, len(pick) - 1) for p in range(len(ROWS))}
    buf, offs, tab = _carve(len(pick))
    c.plan.reconstruct_tasks(dev_pick, tab)
    _check(buf, offs, lambda p, j: c.want[False][pick[j]][p], last)


def test_rows_dev_limits_what_is_read_and_written():
    """rows_dev as svdq_merge_reconstruct reads it: fewer rows than the plan's, and 0 = the parameter is left alone."""
    c = _case("n8-fp16-center")
    plan = c.plan
    rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * plan.P].view(torch.int64)
    assert rows_dev.tolist() == ROWS
    cut = torch.tensor([0 if p == 4 else rows for p, rows in enumerate(ROWS)], dtype=torch.int64).cuda()
    buf, offs, tab = _carve(c.n)
    plan.reconstruct_tasks(list(range(c.n)), tab, rows_dev=cut)
    _check(buf, offs, lambda p, j: c.want[False][j][p], {(4, j) for j in range(c.n)})


# ------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_refused_before_anything_is_launched(sq):
    from ctypes import c_void_p
    nat = sq._native
    c = _case("n8-fp16-center")
    plan, lib = c.plan, nat.lib()
    buf, offs, tab = _carve(c.n)
    idx = torch.arange(c.n, dtype=torch.int32).cuda()
    work = torch.empty(int(lib.svdq_task_reconstruct_work_bytes(plan._h, c.n)), dtype=torch.uint8, device="cuda")
    assert work.numel() >= plan.P * c.n * c.n * 4
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(task_ptr, n_out):
        return lib.svdq_task_reconstruct(plan._h, None, c_void_p(plan.small.data_ptr()), c_void_p(plan.basis.data_ptr()),
                                         c_void_p(plan.mean.data_ptr()), task_ptr, n_out, None, None,
                                         c_void_p(tab.data_ptr()), c_void_p(work.data_ptr()), stream)
    for n_out in (0, 33, -1):
        assert call(c_void_p(idx.data_ptr()), n_out) == nat.SVDQ_EINVAL
        assert "n_out" in nat.last_error()
        assert lib.svdq_task_reconstruct_work_bytes(plan._h, n_out) == 0
    assert call(None, c.n) == nat.SVDQ_EINVAL and "task" in nat.last_error()
    # indices are checked where the host sees them: the call that builds the device table
    for bad in ([0, c.n], [-1], [], list(range(33))):
        with pytest.raises(ValueError, match="svdq_task_reconstruct"):
            plan.reconstruct_tasks(bad, tab)
    with pytest.raises(ValueError, match="out_table"):
        plan.reconstruct_tasks([0, 1], tab)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert call(c_void_p(idx.data_ptr()), c.n) == nat.SVDQ_OK      # the same call, well-formed
    _check(buf, offs, lambda p, j: c.want[False][j][p])


# ------------------------------------------------------------------------------------------ graph capture
def test_capture_and_replay_give_the_eager_bits():
    c = _case("n17-fp16-center")
    pick = list(range(c.n))
    buf, offs, tab = _carve(c.n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.plan.reconstruct_tasks(pick, tab, **c.tables(True))      # warm-up outside the capture: work buffer, task table
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = buf.clone()
    buf.fill_(SENTINEL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c.plan.reconstruct_tasks(pick, tab, **c.tables(True))
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())      # capture does not execute
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager)
    _check(buf, offs, lambda p, j: c.want[True][j][p])
