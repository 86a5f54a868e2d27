"""
GPU tests of the mask operators (csrc/svdq_mask.hip; MaskSet and compute_*_mask in mask_loader.py) against the numpy
model of tests/mask_model.py, which shares nothing with the kernels and is itself anchored on the reference's outputs
(tests/test_mask_model_cpu.py).

Everything here is an integer, a bool byte or a copied fp32 value: every comparison is ``array_equal``, there is no
tolerance in this file.  Every device output the tests can place lives inside a larger buffer of sentinel bytes
(``Guard``): after a call the bytes in front of and behind the output are still the sentinel, and so is the unwritten
tail (entries ``count .. numel``) of an index list or a compacted copy.

What is covered that a comparison between sibling kernels at a handful of shapes is not:
  mask counts   1..32, 33, 64, 255: the second trip of combine_tile's 8-mask loop (from 9), the second trip of the packed
                staging loop (from 16 streams), the limit of the byte-lane vote count (255; 256 is refused)
  thresholds    every vote count 0..n against every threshold, n up to 40
  packed route  all eight bit shifts of every parameter, a first byte at the end / the start of a 16-byte chunk, streams
                that end with their last parameter, 0xFF behind the declared length
  alignment     per-task masks, combined masks and outputs at every residue 1..7 mod 8
  scan / search the carry of the 1024-tile scan, the third level of the 64-ary search, long runs of empty tiles
"""
import numpy as np
import pytest
import torch

import mask_model as mm

pytestmark = pytest.mark.gpu

SENT = 0x5A
GUARD = 64                  # bytes in front of and behind every guarded output (keeps 16-byte alignment)
TILE = 2048                 # MASK_TILE
SIZES = [1, 7, 8, 9, 63, 2047, 2048, 2049, 4096, 4 * 2048 + 1]      # the last: 5 tiles, a second MASK_TPB = 4 block
UNIT_ROWS = 256
N_MASKS = list(range(1, 33)) + [33, 64, 255]
DENSITIES = (0.05, 0.5, 0.95)
THRESHOLDS = [0.0, 0.1, 1 / 3, 0.5, 0.6, 2 / 3, 0.9, 1.0, 1.1]
P3 = [2049, 9, 4 * 2048 + 1]                                          # the parameters of the packed-route layouts
PACKED_N = [1, 15, 16, 17, 32]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


@pytest.fixture(scope="module")
def dev(sq):
    return torch.device("cuda", 0)


def _plan(sizes, unit_rows, dev):
    """A plan only for its work units (row0 = j * unit_rows per parameter): one task, no workspace, no basis."""
    from svdq_amd.pipeline import CompressPlan
    return CompressPlan(sizes, 1, unit_rows=unit_rows, gram_only=True, workspace=False, device=dev)


def _units(plan, sizes, unit_rows):
    per = [-(-D // unit_rows) for D in sizes]
    assert sum(per) == int(plan.sizes.n_units)          # the unit order the starts are read in
    return per


@pytest.fixture(scope="module")
def plan_sizes(sq, dev):
    return _plan(SIZES, UNIT_ROWS, dev)


@pytest.fixture(scope="module")
def plan_p3(sq, dev):
    return _plan(P3, UNIT_ROWS, dev)


# ------------------------------------------------------------------------------------------------ guarded outputs
class Guard:
    """``numel`` elements of ``dtype`` inside a sentinel-filled byte buffer, ``shift`` bytes off the aligned position."""

    def __init__(self, numel, dtype, dev, shift=0):
        self.item = torch.empty(0, dtype=dtype).element_size()
        assert shift % self.item == 0
        self.numel = int(numel)
        self.lo = GUARD + shift
        self.hi = self.lo + self.numel * self.item
        self.buf = torch.full((self.hi + GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.view = self.buf[self.lo:self.hi].view(dtype)

    def get(self, count=None):
        """The first ``count`` elements (all by default) as numpy, after checking that nothing else was written."""
        n = self.numel if count is None else int(count)
        assert 0 <= n <= self.numel, (n, self.numel)
        end = self.lo + n * self.item
        assert bool((self.buf[:self.lo] == SENT).all()), "bytes in front of the output were written"
        assert bool((self.buf[end:] == SENT).all()), "bytes behind the written part of the output were written"
        return self.view[:n].cpu().numpy()

    def untouched(self):
        return bool((self.buf == SENT).all())


def _guards(sizes, dtype, dev, shifts=None):
    return [Guard(D, dtype, dev, shifts[q] if shifts else 0) for q, D in enumerate(sizes)]


def _install(ms, d, key, tab, guards):
    """Point a prepared MaskSet call (``d``: its dict of tensors and pointer tables) at guarded outputs."""
    d[key] = [g.view for g in guards]
    d[tab] = ms._table(d[key])


def _table(tensors, dev):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(dev)


def _u8(mask):
    return np.asarray(mask).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ inputs
def _plant(s, n):
    """Votes that random masks do not produce reliably: a run where every mask is set, a run where none is, and positions
    with exactly ceil(n/2) - 1, ceil(n/2), n/2 and n/2 + 1 votes (which masks vote moves with the position) -- near the
    start, at the end and, where there is one, across the first tile boundary."""
    D = s.shape[1]
    s[:, 3:19] = True
    s[:, 21:37] = False
    half = (n + 1) // 2
    targets = [half - 1, half, n // 2, min(n, n // 2 + 1)]
    planted = {}
    for base in [40, D - 8] + ([TILE - 2] if D >= TILE + 2 else []):
        for i, v in enumerate(targets):
            p = base + i
            s[:, p] = (np.arange(n) + p) % n < v
            planted[p] = v
    return planted


def make_stacks(n, sizes, seed):
    """Per parameter a bool [n, D]: task t has density 0.05 / 0.5 / 0.95 in turn, plus the planted votes."""
    rng = np.random.default_rng(seed)
    dens = np.array([DENSITIES[t % 3] for t in range(n)])
    stacks = []
    for D in sizes:
        s = rng.random((n, D)) < dens[:, None]
        if D >= 64:
            planted = _plant(s, n)
            v = mm.votes(s)
            assert all(v[p] == want for p, want in planted.items())
            assert (v[3:19] == n).all() and (v[21:37] == 0).all()
        stacks.append(s)
    return stacks


def upload_aligned(stacks, dev):
    """Per-task masks as rows of one [n, W] tensor per parameter, W a multiple of 16: every mask starts 16-byte aligned.
    The bytes between the masks are set, so a read past a mask's end would count votes."""
    per_task = []
    for s in stacks:
        n, D = s.shape
        buf = torch.ones((n, -(-D // 16) * 16), dtype=torch.bool, device=dev)
        buf[:, :D] = torch.from_numpy(s).to(dev)
        per_task.append([buf[t, :D] for t in range(n)])
        assert all(m.data_ptr() % 16 == 0 and m.is_contiguous() for m in per_task[-1])
    return per_task


def unaligned_offsets(sizes):
    offs, cur = [], 0
    for q, D in enumerate(sizes):
        while cur % 8 != q % 7 + 1:
            cur += 1
        offs.append(cur)
        cur += D
    return offs, -(-(cur + 1) // 8) * 8


def upload_unaligned(stacks, dev):
    """What a tall mask turns into: ONE flat bool tensor per task, parameter q a view ``flat[o_q : o_q + D_q]`` of it;
    the offsets take every residue 1..7 mod 8.  The bytes between the parameters are set."""
    sizes = [s.shape[1] for s in stacks]
    offs, total = unaligned_offsets(sizes)
    n = stacks[0].shape[0]
    flat = np.ones((n, total), dtype=np.bool_)
    for o, s in zip(offs, stacks):
        flat[:, o:o + s.shape[1]] = s
    buf = torch.from_numpy(flat).to(dev)
    per_task = [[buf[t, o:o + D] for t in range(n)] for o, D in zip(offs, sizes)]
    res = {m.data_ptr() % 8 for ms_ in per_task for m in ms_}
    assert res == set(range(1, 8)) if len(sizes) >= 7 else 0 not in res, res
    return per_task


def pack_streams(stacks, dev):
    """numpy.packbits streams (one per task over the concatenated parameters), 16-byte aligned, 0xFF behind each."""
    n = stacks[0].shape[0]
    flat = np.concatenate(stacks, axis=1)
    packed = np.packbits(flat, axis=1)
    nbytes = packed.shape[1]
    host = np.full((n, (nbytes // 16 + 2) * 16), 0xFF, dtype=np.uint8)
    host[:, :nbytes] = packed
    buf = torch.from_numpy(host).to(dev)
    offs = np.concatenate([[0], np.cumsum([s.shape[1] for s in stacks])[:-1]]).tolist()
    return [buf[t, :nbytes] for t in range(n)], offs


# ------------------------------------------------------------------------------------------------ routes
def mask_combine_guarded(sq, masks, code, dev, shift=0):
    """svdq_mask_combine through the C ABI, output and count inside guards (compute_*_mask allocate their own)."""
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import _ptr, _stream_ptr
    lib = nat.lib()
    numel = masks[0].numel()
    table = _table(masks, dev)
    out, cnt = Guard(numel, torch.uint8, dev, shift), Guard(1, torch.int64, dev)
    work = torch.empty(int(lib.svdq_mask_work_bytes(numel)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.svdq_mask_combine(_ptr(table), len(masks), numel, code, _ptr(out.view), _ptr(cnt.view), _ptr(work),
                                        _stream_ptr()), "svdq_mask_combine")
    torch.cuda.synchronize()
    return out, cnt


def _check_masks(outs, want, what):
    got = [o.get() for o in outs]
    for q, w in enumerate(want):
        assert np.array_equal(got[q], _u8(w)), (what, q)
    return got


def _check_lists(its, ifs, want, what):
    got = []
    for q, w in enumerate(want):
        t, f = mm.indices(w)
        a, b = its[q].get(t.size), ifs[q].get(f.size)
        assert np.array_equal(a, t) and np.array_equal(b, f), (what, q)
        got += [a, b]
    return got


def _model_starts(masks, rows, per, unit_rows, inverted):
    return np.concatenate([mm.unit_starts(m, int(rows[q]), per[q], unit_rows, inverted) for q, m in enumerate(masks)])


def run_bool_routes(sq, plan, per_task, stacks, out_shifts=None, streams=None):
    """Every route that combines bool-byte masks (and, given ``streams``, the bit-packed ones) for the three strategies
    against the model.  Returns what the device wrote, for a bit-for-bit comparison between input layouts."""
    from svdq_amd import _native as nat
    from svdq_amd.mask_loader import MaskSet
    dev = per_task[0][0].device
    sizes = [s.shape[1] for s in stacks]
    Q, n = len(sizes), stacks[0].shape[0]
    per = _units(plan, sizes, UNIT_ROWS)
    ms = MaskSet(sizes, dev)
    fns = {"union": sq.compute_union_mask, "intersection": sq.compute_intersection_mask,
           "majority": sq.compute_majority_mask}
    res = {}
    for strat in mm.STRATEGIES:
        want = [mm.combine(s, strat) for s in stacks]
        cnt = np.array([w.sum() for w in want], dtype=np.int64)
        cntf = np.array(sizes, dtype=np.int64) - cnt
        wstarts = _model_starts(want, cnt, per, UNIT_ROWS, False)
        r = res[strat] = []

        def mask_guards():
            return _guards(sizes, torch.uint8, dev, out_shifts)

        # one parameter at a time: compute_*_mask, and the entry point below it with a guarded output
        for q in range(Q):
            got = fns[strat](per_task[q])
            assert got.dtype == torch.bool and got.device == per_task[q][0].device
            assert np.array_equal(got.cpu().numpy(), want[q]), (strat, q)
            out, c = mask_combine_guarded(sq, per_task[q], nat.MASK_STRATEGIES[strat], dev,
                                          out_shifts[q] if out_shifts else 0)
            assert np.array_equal(out.get(), _u8(want[q])) and int(c.get()[0]) == cnt[q], (strat, q)
        # MaskSet.combine
        ms.prepare_combine(per_task, strat)
        outs = mask_guards()
        _install(ms, ms._c, "outs", "ot", outs)
        ms.run_combine()
        torch.cuda.synchronize()
        r += _check_masks(outs, want, (strat, "combine"))
        assert np.array_equal(ms._c["counts"].cpu().numpy(), cnt), strat
        # combine + index lists in three launches
        ms.prepare_combine_indices(per_task, strat, want_false=True)
        outs, its, ifs = mask_guards(), _guards(sizes, torch.int32, dev), _guards(sizes, torch.int32, dev)
        _install(ms, ms._c, "outs", "ot", outs)
        _install(ms, ms._i, "it", "tt", its)
        _install(ms, ms._i, "if_", "ft", ifs)
        ms.run_combine_indices()
        torch.cuda.synchronize()
        r += _check_masks(outs, want, (strat, "combine_indices"))
        r += _check_lists(its, ifs, want, (strat, "combine_indices"))
        assert np.array_equal(ms._i["ct"].cpu().numpy(), cnt) and np.array_equal(ms._i["cf"].cpu().numpy(), cntf)
        # combine + scan + unit starts in three launches
        ms.prepare_combine_starts(per_task, strat, plan)
        outs, us = mask_guards(), Guard(sum(per), torch.int64, dev)
        _install(ms, ms._c, "outs", "ot", outs)
        ms._cs["us"] = us.view
        ms.run_combine_starts()
        torch.cuda.synchronize()
        r += _check_masks(outs, want, (strat, "combine_starts"))
        assert np.array_equal(ms._cs["ct"].cpu().numpy(), cnt) and np.array_equal(ms._cs["cf"].cpu().numpy(), cntf)
        got = us.get()
        assert np.array_equal(got, wstarts), (strat, "combine_starts")
        r.append(got)
        if streams is None:
            continue
        st, offs = streams
        # the same from bit-packed streams
        ms.prepare_combine_packed_indices(st, offs, strat, want_false=True)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(ms._p["st"], st))      # read in place: 0xFF follows
        outs, its, ifs = mask_guards(), _guards(sizes, torch.int32, dev), _guards(sizes, torch.int32, dev)
        _install(ms, ms._p, "outs", "ot", outs)
        _install(ms, ms._p, "it", "tt", its)
        _install(ms, ms._p, "if_", "ft", ifs)
        ms.run_combine_packed_indices()
        torch.cuda.synchronize()
        _check_masks(outs, want, (strat, "combine_packed_indices"))
        _check_lists(its, ifs, want, (strat, "combine_packed_indices"))
        assert np.array_equal(ms._p["ct"].cpu().numpy(), cnt) and np.array_equal(ms._p["cf"].cpu().numpy(), cntf)
        ms.prepare_combine_packed_starts(st, offs, strat, plan)
        outs, us = mask_guards(), Guard(sum(per), torch.int64, dev)
        _install(ms, ms._ps, "outs", "ot", outs)
        ms._ps["us"] = us.view
        ms.run_combine_packed_starts()
        torch.cuda.synchronize()
        _check_masks(outs, want, (strat, "combine_packed_starts"))
        assert np.array_equal(ms._ps["ct"].cpu().numpy(), cnt) and np.array_equal(ms._ps["cf"].cpu().numpy(), cntf)
        assert np.array_equal(us.get(), wstarts), (strat, "combine_packed_starts")
    ms.close()
    return res


def unit_starts_guarded(ms, plan, rows_dev, entry_map, mask_table):
    """svdq_maskset_unit_starts with the starts inside a guard (MaskSet.unit_starts allocates its own)."""
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import _ptr, _stream_ptr
    em = None
    if entry_map is not None:
        em = torch.tensor([int(q) - (1 << 31) if inv else int(q) for q, inv in entry_map],
                          dtype=torch.int32).to(ms.device)
    us = Guard(int(plan.sizes.n_units), torch.int64, ms.device)
    with torch.cuda.device(ms.device):
        nat.check(ms.lib.svdq_maskset_unit_starts(ms._h, plan._h, _ptr(mask_table), _ptr(em), _ptr(rows_dev),
                                                  _ptr(ms.work), _ptr(us.view), _stream_ptr()),
                  "svdq_maskset_unit_starts")
    torch.cuda.synchronize()
    return us.get()


def check_indices(ms, masks_dev, masks_np):
    sizes = ms.numels
    ms.prepare_indices(masks_dev, want_false=True)
    its, ifs = _guards(sizes, torch.int32, ms.device), _guards(sizes, torch.int32, ms.device)
    _install(ms, ms._i, "it", "tt", its)
    _install(ms, ms._i, "if_", "ft", ifs)
    ms.run_indices()
    torch.cuda.synchronize()
    _check_lists(its, ifs, masks_np, "indices")
    cnt = np.array([m.sum() for m in masks_np], dtype=np.int64)
    assert np.array_equal(ms._i["ct"].cpu().numpy(), cnt)
    assert np.array_equal(ms._i["cf"].cpu().numpy(), np.array(sizes, dtype=np.int64) - cnt)


def _sources(D, n_src):
    """fp32 values that name their position: i + 1, -(i + 1), (i + 1) / 2 -- exact in fp32 below 2^24 elements."""
    assert D < (1 << 24)
    x = np.arange(1, D + 1, dtype=np.float32)
    return [x, -x, x * np.float32(0.5)][:n_src]


def check_compact(ms, masks_dev, masks_np, n_src):
    dev, sizes = ms.device, ms.numels
    src_np = [_sources(D, n_src) for D in sizes]
    srcs = [[torch.from_numpy(x).to(dev) for x in xs] for xs in src_np]
    ms.prepare_compact(masks_dev, srcs, want_false=True)
    dt = [_guards([D] * n_src, torch.float32, dev) for D in sizes]
    df = [_guards([D] * n_src, torch.float32, dev) for D in sizes]
    ms._x["tt"] = ms._table([g.view for gs in dt for g in gs])
    ms._x["ft"] = ms._table([g.view for gs in df for g in gs])
    ms.run_compact()
    torch.cuda.synchronize()
    for q, m in enumerate(masks_np):
        for s in range(n_src):
            t, f = mm.compact(src_np[q][s], m)
            assert np.array_equal(dt[q][s].get(t.size), t), ("compact", q, s, "selected")
            assert np.array_equal(df[q][s].get(f.size), f), ("compact", q, s, "cleared")
    cnt = np.array([m.sum() for m in masks_np], dtype=np.int64)
    assert np.array_equal(ms._x["ct"].cpu().numpy(), cnt)
    assert np.array_equal(ms._x["cf"].cpu().numpy(), np.array(sizes, dtype=np.int64) - cnt)


def check_count_scan_and_starts(ms, masks_dev, masks_np, plan, unit_rows):
    sizes = ms.numels
    per = _units(plan, sizes, unit_rows)
    ct, cf = ms.count_scan(masks_dev)
    cnt = np.array([m.sum() for m in masks_np], dtype=np.int64)
    cntf = np.array(sizes, dtype=np.int64) - cnt
    assert np.array_equal(ct.cpu().numpy(), cnt) and np.array_equal(cf.cpu().numpy(), cntf)
    mt = ms._s["mt"]
    for inv, rows_dev, rows in ((False, ct, cnt), (True, cf, cntf)):
        em = [(q, inv) for q in range(len(sizes))]
        want = _model_starts(masks_np, rows, per, unit_rows, inv)
        assert np.array_equal(unit_starts_guarded(ms, plan, rows_dev, em, mt), want), (unit_rows, inv)
        assert np.array_equal(ms.unit_starts(plan, rows_dev, entry_map=em).cpu().numpy(), want), (unit_rows, inv)
    want = _model_starts(masks_np, cnt, per, unit_rows, False)
    assert np.array_equal(unit_starts_guarded(ms, plan, ct, None, mt), want), (unit_rows, "identity map")


# ------------------------------------------------------------------------------------------------ (a) every mask count
@pytest.mark.parametrize("n_masks", N_MASKS)
def test_every_mask_count(sq, dev, plan_sizes, n_masks):
    """1..32, 33, 64 and 255 masks through every combining route, all three strategies."""
    stacks = make_stacks(n_masks, SIZES, 1000 + n_masks)
    run_bool_routes(sq, plan_sizes, upload_aligned(stacks, dev), stacks,
                    streams=pack_streams(stacks, dev) if n_masks <= 32 else None)


# ------------------------------------------------------------------------------------------------ (b) thresholds
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 16, 17, 32, 40])
def test_custom_thresholds(sq, dev, n):
    """Position p has exactly p mod (n + 1) votes (mask t votes iff t < that), so every vote count 0..n occurs, also on
    both sides of the tile boundary; every threshold against the reference's fp32 rule."""
    D = TILE + 64
    v = np.arange(D) % (n + 1)
    stack = np.arange(n)[:, None] < v[None, :]
    assert np.array_equal(mm.votes(stack), v)
    assert set(v[:TILE]) == set(range(n + 1)) and len(set(v[TILE - 1:TILE + 1])) == 2
    masks = [torch.from_numpy(stack[t].copy()).to(dev) for t in range(n)]
    for thr in THRESHOLDS:
        got = sq.compute_majority_mask(masks, threshold=thr)
        assert got.dtype == torch.bool
        assert np.array_equal(got.cpu().numpy(), mm.majority_threshold(stack, thr)), (n, thr)


# ------------------------------------------------------------------------------------------------ (c) packed route
def _vote_levels(rng, n, nbits):
    """Bits whose vote count is informative at every n: each position draws a level (never / rarely / half / mostly /
    always set) and every task follows it, so union has cleared and intersection has set elements up to 32 streams."""
    level = rng.choice(np.array([0.0, 0.03, 0.5, 0.97, 1.0]), size=nbits)
    return rng.random((n, nbits)) < level[None, :]


@pytest.mark.parametrize("first_byte", [15, 16])
@pytest.mark.parametrize("pad", range(8))
def test_packed_shifts_chunk_edges_stream_ends(sq, dev, plan_p3, pad, first_byte):
    """The first parameter at bit ``pad`` of stream byte 15 (the last of a 16-byte chunk) or 16; 0..7 pad bits in front
    of the second and of the third parameter; the stream ends with the last parameter's last bit, mid-chunk, and 0xFF
    follows.  1, 15, 16, 17 and 32 streams, three strategies."""
    from svdq_amd.mask_loader import MaskSet
    rng = np.random.default_rng(100 * first_byte + pad)
    pool = _vote_levels(rng, 32, 8 * (first_byte + 1290))
    ms = MaskSet(P3, dev)
    per = _units(plan_p3, P3, UNIT_ROWS)
    shifts = set()
    for g in range(8):
        o0 = 8 * first_byte + pad
        o1 = o0 + P3[0] + g
        o2 = o1 + P3[1] + (2 * g + pad) % 8          # o2 & 7 = 2 pad + 2 + 3 g mod 8: every shift as g runs
        offs = [o0, o1, o2]
        nbytes = (o2 + P3[2] + 7) // 8          # exactly the bytes the parameters need
        assert (o0 >> 3, o0 & 7) == (first_byte, pad) and nbytes % 16 != 0 and 8 * nbytes <= pool.shape[1]
        shifts.add((o1 & 7, o2 & 7))
        packed = np.packbits(pool[:, :8 * nbytes], axis=1)
        host = np.full((32, (nbytes // 16 + 3) * 16), 0xFF, dtype=np.uint8)
        host[:, :nbytes] = packed
        buf = torch.from_numpy(host).to(dev)
        stacks = [np.stack([mm.unpack(packed[t], o, D) for t in range(32)]) for o, D in zip(offs, P3)]
        for n in PACKED_N:
            streams = [buf[t, :nbytes] for t in range(n)]
            assert all(s.data_ptr() % 16 == 0 for s in streams)
            for strat in mm.STRATEGIES:
                want = [mm.combine(s[:n], strat) for s in stacks]
                cnt = np.array([w.sum() for w in want], dtype=np.int64)
                what = (pad, first_byte, g, n, strat)
                ms.prepare_combine_packed_indices(streams, offs, strat, want_false=True)
                assert all(a.data_ptr() == b.data_ptr() for a, b in zip(ms._p["st"], streams))
                outs, its, ifs = (_guards(P3, torch.uint8, dev), _guards(P3, torch.int32, dev),
                                  _guards(P3, torch.int32, dev))
                _install(ms, ms._p, "outs", "ot", outs)
                _install(ms, ms._p, "it", "tt", its)
                _install(ms, ms._p, "if_", "ft", ifs)
                ms.run_combine_packed_indices()
                torch.cuda.synchronize()
                _check_masks(outs, want, what)
                _check_lists(its, ifs, want, what)
                assert np.array_equal(ms._p["ct"].cpu().numpy(), cnt), what
                if g:
                    continue
                ms.prepare_combine_packed_starts(streams, offs, strat, plan_p3)
                outs, us = _guards(P3, torch.uint8, dev), Guard(sum(per), torch.int64, dev)
                _install(ms, ms._ps, "outs", "ot", outs)
                ms._ps["us"] = us.view
                ms.run_combine_packed_starts()
                torch.cuda.synchronize()
                _check_masks(outs, want, what)
                assert np.array_equal(us.get(), _model_starts(want, cnt, per, UNIT_ROWS, False)), what
    assert {a for a, _ in shifts} == set(range(8)) and {b for _, b in shifts} == set(range(8))
    ms.close()


def test_packed_refusals(sq, dev, plan_p3):
    from svdq_amd import _native as nat
    from svdq_amd.mask_loader import MaskSet
    rng = np.random.default_rng(5)
    offs = [0, P3[0], P3[0] + P3[1]]
    nbytes = (sum(P3) + 7) // 8
    buf = torch.from_numpy(rng.integers(0, 256, (33, (nbytes // 16 + 1) * 16), dtype=np.uint8)).to(dev)
    ms = MaskSet(P3, dev)
    for prepare, args in ((ms.prepare_combine_packed_indices, (False,)), (ms.prepare_combine_packed_starts, (plan_p3,))):
        with pytest.raises(ValueError, match="shorter than the parameters"):
            prepare([buf[t, :nbytes - 1] for t in range(3)], offs, "union", *args)
        with pytest.raises(ValueError, match="Empty mask list"):
            prepare([], offs, "union", *args)
    streams = [buf[t, :nbytes] for t in range(33)]
    ms.prepare_combine_packed_indices(streams, offs, "union", want_false=True)
    outs, its, ifs = _guards(P3, torch.uint8, dev), _guards(P3, torch.int32, dev), _guards(P3, torch.int32, dev)
    _install(ms, ms._p, "outs", "ot", outs)
    _install(ms, ms._p, "it", "tt", its)
    _install(ms, ms._p, "if_", "ft", ifs)
    with pytest.raises(ValueError, match="at most 32 packed mask streams"):
        ms.run_combine_packed_indices()
    ms.prepare_combine_packed_starts(streams, offs, "union", plan_p3)
    outs2, us = _guards(P3, torch.uint8, dev), Guard(int(plan_p3.sizes.n_units), torch.int64, dev)
    _install(ms, ms._ps, "outs", "ot", outs2)
    ms._ps["us"] = us.view
    with pytest.raises(ValueError, match="at most 32 packed mask streams"):
        ms.run_combine_packed_starts()
    assert "32" in nat.last_error()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs + its + ifs + outs2 + [us])
    ms.close()


# ------------------------------------------------------------------------------------------------ (d) unaligned views
@pytest.mark.parametrize("n_masks", [3, 9, 20])
def test_unaligned_mask_views(sq, dev, plan_sizes, n_masks):
    """Per-task masks as views into one flat bool tensor per task (every residue 1..7 mod 8), combined masks written at
    unaligned addresses: the model's result, and bit for bit what the aligned layout gives.  Then the combined masks,
    again as unaligned views of one flat buffer, through indices, compact, count / scan and unit starts."""
    from svdq_amd.mask_loader import MaskSet
    stacks = make_stacks(n_masks, SIZES, 2000 + n_masks)
    streams = pack_streams(stacks, dev)
    aligned = run_bool_routes(sq, plan_sizes, upload_aligned(stacks, dev), stacks, streams=streams)
    shifts = [q % 7 + 1 for q in range(len(SIZES))]
    views = run_bool_routes(sq, plan_sizes, upload_unaligned(stacks, dev), stacks, out_shifts=shifts, streams=streams)
    for strat in mm.STRATEGIES:
        assert len(aligned[strat]) == len(views[strat])
        for a, b in zip(aligned[strat], views[strat]):
            assert a.dtype == b.dtype and np.array_equal(a, b), strat
    for strat in ("majority", "union"):
        comb = [mm.combine(s, strat) for s in stacks]
        masks_dev = [ms_[0] for ms_ in upload_unaligned([c[None, :] for c in comb], dev)]
        assert {m.data_ptr() % 8 for m in masks_dev} == set(range(1, 8))
        ms = MaskSet(SIZES, dev)
        check_indices(ms, masks_dev, comb)
        check_compact(ms, masks_dev, comb, 2)
        check_count_scan_and_starts(ms, masks_dev, comb, plan_sizes, UNIT_ROWS)
        ms.close()


def test_unaligned_packed_stream_is_copied(sq, dev):
    """A packed stream whose address is not a multiple of 16 (``buf[1:]``) gives what the aligned stream gives."""
    from svdq_amd.mask_loader import MaskSet
    stacks = make_stacks(5, P3, 77)
    (st, offs) = pack_streams(stacks, dev)
    nbytes = st[0].numel()
    odd = []
    for t, s in enumerate(st):
        buf = torch.full((nbytes + 1 + t,), 0xFF, dtype=torch.uint8, device=dev)
        buf[1 + t:] = s
        odd.append(buf[1 + t:])
    assert all(s.data_ptr() % 16 != 0 for s in odd)
    ms = MaskSet(P3, dev)
    for strat in mm.STRATEGIES:
        want = [mm.combine(s, strat) for s in stacks]
        ms.prepare_combine_packed_indices(odd, offs, strat, want_false=True)
        assert all(s.data_ptr() % 16 == 0 for s in ms._p["st"])
        outs, its, ifs = _guards(P3, torch.uint8, dev), _guards(P3, torch.int32, dev), _guards(P3, torch.int32, dev)
        _install(ms, ms._p, "outs", "ot", outs)
        _install(ms, ms._p, "it", "tt", its)
        _install(ms, ms._p, "if_", "ft", ifs)
        ms.run_combine_packed_indices()
        torch.cuda.synchronize()
        _check_masks(outs, want, strat)
        _check_lists(its, ifs, want, strat)
    ms.close()


# ------------------------------------------------------------------------------------------------ (e) structured masks
T5 = 5 * TILE + 3
ALT = 4                       # index of the alternating mask
BIG_CARRY = 1024 * TILE + 2 * TILE + 5          # more than 1024 tiles: the scan carries into a second chunk
BIG_SEARCH = 4097 * TILE + 11                   # more than 4096 tiles: a third level of the 64-ary search


def _structured():
    rng = np.random.default_rng(11)
    masks = [np.zeros(T5, dtype=np.bool_) for _ in range(9)]
    masks[0][:] = True                           # all set
    #     1                                        none set
    masks[2][0] = True                           # only element 0
    masks[3][-1] = True                          # only the last element
    masks[ALT][::2] = True                       # alternating
    masks[5][:] = True
    masks[5][:3 * TILE] = False                  # tiles 0-2 empty
    masks[6][:] = True
    masks[6][TILE:4 * TILE] = False              # tiles 1-3 empty
    masks[7][:] = True
    masks[7][4 * TILE:] = False                  # the last two tiles empty (the fifth full one and the 3-element tail)
    masks[8][2 * TILE:3 * TILE] = True           # exactly one full tile set
    masks.append(rng.random(BIG_CARRY) < 0.5)
    big = rng.random(BIG_SEARCH) < 0.03
    big[100 * TILE:164 * TILE] = False           # tiles 100-163 cleared: off(i) flat over a whole search level
    masks.append(big)
    return masks


class Structured:
    def __init__(self, dev):
        from svdq_amd.mask_loader import MaskSet
        self.np = _structured()
        self.sizes = [m.size for m in self.np]
        assert self.sizes == [T5] * 9 + [BIG_CARRY, BIG_SEARCH]
        self.dev = [torch.from_numpy(m).to(dev) for m in self.np]
        self.ms = MaskSet(self.sizes, dev)


@pytest.fixture(scope="module")
def structured(sq, dev):
    s = Structured(dev)
    yield s
    s.ms.close()


def test_structured_indices(structured):
    check_indices(structured.ms, structured.dev, structured.np)


@pytest.mark.parametrize("n_src", [1, 3])
def test_structured_compact(structured, n_src):
    check_compact(structured.ms, structured.dev, structured.np, n_src)


@pytest.mark.parametrize("unit_rows", [256, 1024, 2048])
def test_structured_count_scan_and_unit_starts(structured, dev, unit_rows):
    plan = _plan(structured.sizes, unit_rows, dev)
    check_count_scan_and_starts(structured.ms, structured.dev, structured.np, plan, unit_rows)


def test_unit_starts_when_counts_and_mask_disagree(structured, dev):
    """rows_dev 300 above the true count of one parameter: its units whose first row lies at or past the true count find
    no element and get numel | tag; every other start is unchanged."""
    ms, sizes = structured.ms, structured.sizes
    plan = _plan(sizes, UNIT_ROWS, dev)
    per = _units(plan, sizes, UNIT_ROWS)
    ct, cf = ms.count_scan(structured.dev)
    for inv, counts in ((False, ct), (True, cf)):
        true = counts.cpu().numpy()
        rows = true.copy()
        rows[ALT] += 300
        r0 = np.arange(per[ALT]) * UNIT_ROWS
        hit = (r0 >= true[ALT]) & (r0 < rows[ALT])
        assert hit.any()                                                    # the branch is reached
        want = _model_starts(structured.np, rows, per, UNIT_ROWS, inv)
        u0 = sum(per[:ALT])
        tag = mm.WALK_INV if inv else 0
        assert (want[u0:u0 + per[ALT]][hit] == (sizes[ALT] | tag)).all()
        rows_dev = torch.from_numpy(rows).to(dev)
        em = [(q, inv) for q in range(len(sizes))]
        assert np.array_equal(unit_starts_guarded(ms, plan, rows_dev, em, ms._s["mt"]), want), inv


# ------------------------------------------------------------------------------------------------ (f) limits
def test_more_than_255_bool_masks_are_refused(sq, dev, plan_sizes):
    """The byte-lane vote count holds 255 (test_every_mask_count[255]); 256 masks are refused by all four bool routes
    before anything is launched, with an error that names the limit."""
    from svdq_amd import _native as nat
    from svdq_amd.mask_loader import MaskSet
    stacks = make_stacks(1, SIZES, 9)
    one = upload_aligned(stacks, dev)
    per_task = [[ms_[0]] * 256 for ms_ in one]
    for strat in mm.STRATEGIES:
        with pytest.raises(ValueError, match="at most 255 bool masks"):
            mask_combine_guarded(sq, per_task[-1], nat.MASK_STRATEGIES[strat], dev)
        assert "255" in nat.last_error()
    for fn in (sq.compute_union_mask, sq.compute_intersection_mask, sq.compute_majority_mask):
        with pytest.raises(ValueError, match="at most 255 bool masks"):
            fn(per_task[-1])
    with pytest.raises(ValueError, match="at most 255 bool masks"):
        sq.compute_majority_mask(per_task[-1], threshold=0.9)
    # the refusal comes before the launch: a guarded output stays untouched
    lib = nat.lib()
    from svdq_amd.pipeline import _ptr, _stream_ptr
    out, cnt = Guard(SIZES[-1], torch.uint8, dev), Guard(1, torch.int64, dev)
    table = _table(per_task[-1], dev)
    rc = lib.svdq_mask_combine(_ptr(table), 256, SIZES[-1], 0, _ptr(out.view), _ptr(cnt.view), None, _stream_ptr())
    assert rc == nat.SVDQ_EINVAL and "255" in nat.last_error()
    torch.cuda.synchronize()
    assert out.untouched() and cnt.untouched()
    ms = MaskSet(SIZES, dev)
    n_units = int(plan_sizes.sizes.n_units)
    for strat in mm.STRATEGIES:
        guards = []
        ms.prepare_combine(per_task, strat)
        outs = _guards(SIZES, torch.uint8, dev)
        _install(ms, ms._c, "outs", "ot", outs)
        with pytest.raises(ValueError, match="svdq_maskset_combine: at most 255 bool masks"):
            ms.run_combine()
        guards += outs
        ms.prepare_combine_indices(per_task, strat, want_false=True)
        outs, its, ifs = _guards(SIZES, torch.uint8, dev), _guards(SIZES, torch.int32, dev), _guards(SIZES, torch.int32, dev)
        _install(ms, ms._c, "outs", "ot", outs)
        _install(ms, ms._i, "it", "tt", its)
        _install(ms, ms._i, "if_", "ft", ifs)
        with pytest.raises(ValueError, match="svdq_maskset_combine_indices: at most 255 bool masks"):
            ms.run_combine_indices()
        guards += outs + its + ifs
        ms.prepare_combine_starts(per_task, strat, plan_sizes)
        outs, us = _guards(SIZES, torch.uint8, dev), Guard(n_units, torch.int64, dev)
        _install(ms, ms._c, "outs", "ot", outs)
        ms._cs["us"] = us.view
        with pytest.raises(ValueError, match="svdq_maskset_combine_starts: at most 255 bool masks"):
            ms.run_combine_starts()
        guards += outs + [us]
        torch.cuda.synchronize()
        assert all(g.untouched() for g in guards), strat
    ms.close()


def test_empty_mask_list(sq, dev):
    from svdq_amd.mask_loader import MaskSet
    for fn in (sq.compute_union_mask, sq.compute_intersection_mask, sq.compute_majority_mask):
        with pytest.raises(ValueError, match="Empty mask list"):
            fn([])
    with pytest.raises(ValueError, match="Empty mask list"):
        sq.compute_majority_mask([], threshold=0.9)
    ms = MaskSet(SIZES, dev)
    for strat in mm.STRATEGIES:
        with pytest.raises(ValueError, match="Empty mask list"):
            ms.prepare_combine([[] for _ in SIZES], strat)
        with pytest.raises(ValueError, match="Empty mask list"):
            ms.prepare_combine_indices([[] for _ in SIZES], strat, want_false=True)
    ms.close()
