"""
GPU tests of the single-parameter mask operators (csrc/svdq_mask.hip: svdq_mask_compact with both polarities,
svdq_mask_expand, the count of svdq_mask_combine) against numpy: ``x[m]``, ``x[~m]`` and
``out = zeros; out[m] = sig; out[~m] = noise``.  The set-level operators are held by tests/test_hip_mask_ops.py; this
file is its counterpart for the entry points that take one mask.

The C entry points are called directly, so that unaligned mask, source and output pointers reach the kernels (the
Python wrappers copy their inputs into fresh, aligned tensors).  Every output lives in a sentinel-filled buffer
(``Guard`` of test_hip_mask_ops.py): the bytes around it and the unwritten tail ``count .. numel`` of a compacted copy
stay the sentinel.  fp32 values are only copied, so every comparison is ``array_equal`` on their bit patterns.

  sizes      one thread, one 8-element slice and its neighbours, one tile (2048) and its neighbours, two tiles, a fifth
             tile, and 1025 tiles + 3: the carry of the 1024-tile scan into a second chunk
  densities  0, 0.05, 0.5, 0.95, 1: empty and full tiles, empty and full outputs
  runs       many empty tiles in front of a full one (and, inverted, full ones in front of an empty one)
  alignment  mask pointer at every residue 1..7 mod 8, source and output pointers at 4, 8 and 12 mod 16
"""
import functools

import numpy as np
import pytest
import torch

from test_hip_mask_ops import GUARD, SENT, SIZES, TILE, Guard, mask_combine_guarded

pytestmark = pytest.mark.gpu

BIG_CARRY = 1025 * TILE + 3
ALL_SIZES = SIZES + [BIG_CARRY]
DENSITIES = (0.0, 0.05, 0.5, 0.95, 1.0)
N_SRC_MAX = 3
assert GUARD % 16 == 0 and SENT != 0 and ALL_SIZES[:10] == [1, 7, 8, 9, 63, 2047, 2048, 2049, 4096, 4 * 2048 + 1]


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    assert torch.cuda.is_available()
    return svdq_amd


@pytest.fixture(scope="module")
def dev(sq):
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=8)
def _host_case(numel, density):
    """(three fp32 sources, bool mask) for one size and density; computed once, never modified."""
    rng = np.random.default_rng([numel, int(100 * density)])
    xs = [rng.standard_normal(numel, dtype=np.float32) for _ in range(N_SRC_MAX)]
    xs[0][::5] = -0.0                      # bit patterns a value comparison would not tell apart
    m = rng.random(numel) < density
    assert density not in (0.0, 1.0) or m.all() == (density == 1.0)
    for a in xs + [m]:
        a.setflags(write=False)
    return xs, m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def place(host, dev, shift=0, pad=0x01):
    """``host`` on the device, ``shift`` bytes behind a 256-byte aligned address, ``pad`` bytes around it: a set mask
    byte (or a non-zero float) is what a read past either end would pick up."""
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    buf = np.full(256 + shift + raw.size + 256, pad, dtype=np.uint8)
    buf[256 + shift:256 + shift + raw.size] = raw
    t = torch.from_numpy(buf).to(dev)
    assert t.data_ptr() % 256 == 0
    view = t[256 + shift:256 + shift + raw.size]
    return view.view(torch.bool if host.dtype == np.bool_ else torch.float32)


def _table(tensors, dev):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(dev)


# ------------------------------------------------------------------------------------------------ the entry points
def compact(dev, srcs, mask, invert, out_shifts=None):
    """svdq_mask_compact -> (guarded outputs, count)."""
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import _ptr, _stream_ptr
    lib = nat.lib()
    numel = mask.numel()
    outs = [Guard(numel, torch.float32, dev, out_shifts[i] if out_shifts else 0) for i in range(len(srcs))]
    cnt = Guard(1, torch.int64, dev)
    stab, dtab = _table(srcs, dev), _table([g.view for g in outs], dev)
    work = torch.empty(int(lib.svdq_mask_work_bytes(numel)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.svdq_mask_compact(_ptr(stab), _ptr(dtab), len(srcs), _ptr(mask), int(invert), numel,
                                        _ptr(cnt.view), _ptr(work), _stream_ptr()), "svdq_mask_compact")
    torch.cuda.synchronize()
    return outs, int(cnt.get()[0])


def expand(dev, sig, noise, mask, out_shift=0):
    """svdq_mask_expand -> guarded output."""
    from svdq_amd import _native as nat
    from svdq_amd.pipeline import _ptr, _stream_ptr
    lib = nat.lib()
    numel = mask.numel()
    out = Guard(numel, torch.float32, dev, out_shift)
    work = torch.empty(int(lib.svdq_mask_work_bytes(numel)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.svdq_mask_expand(_ptr(sig), _ptr(noise), _ptr(mask), numel, _ptr(out.view), _ptr(work),
                                       _stream_ptr()), "svdq_mask_expand")
    torch.cuda.synchronize()
    return out


def check_compact(dev, xs, m, mask_shift=0, src_shifts=None, out_shifts=None):
    """Both polarities of one mask over ``len(xs)`` sources; returns the guarded outputs of the first source."""
    srcs = [place(x, dev, src_shifts[i] if src_shifts else 0) for i, x in enumerate(xs)]
    mask = place(m, dev, mask_shift)
    assert mask.data_ptr() % 8 == mask_shift % 8
    first = []
    for invert in (False, True):
        sel = ~m if invert else m
        outs, count = compact(dev, srcs, mask, invert, out_shifts)
        assert count == int(sel.sum()), (invert, count, int(sel.sum()))
        for x, g in zip(xs, outs):
            assert np.array_equal(_bits(g.get(count)), _bits(x[sel])), (invert, m.size)   # get(): the tail is sentinel
        first.append(outs[0])
    return first


def model_expand(sig, noise, m):
    out = np.zeros(m.size, dtype=np.float32)
    out[m] = sig
    if noise is not None:
        out[~m] = noise
    return out


def check_expand(dev, x, m, mask_shift=0, out_shift=0):
    """With and without noise, from numpy's compaction (one spare element: no empty buffer at density 0 or 1)."""
    mask = place(m, dev, mask_shift)
    spare = np.full(1, 7.0, dtype=np.float32)
    sig, noise = place(np.concatenate([x[m], spare]), dev, 0, 0x7F), place(np.concatenate([x[~m], spare]), dev, 0, 0x7F)
    for noi in (noise, None):
        out = expand(dev, sig, noi, mask, out_shift)
        want = model_expand(x[m], None if noi is None else x[~m], m)
        assert np.array_equal(_bits(out.get()), _bits(want)), (m.size, noi is None)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("n_src", [1, 3])
@pytest.mark.parametrize("numel", ALL_SIZES)
def test_compact_sizes_densities_polarities(sq, dev, numel, n_src):
    for density in DENSITIES:
        xs, m = _host_case(numel, density)
        check_compact(dev, xs[:n_src], m)


@pytest.mark.parametrize("numel", ALL_SIZES)
def test_expand_and_round_trip(sq, dev, numel):
    for density in DENSITIES:
        xs, m = _host_case(numel, density)
        x = xs[0]
        check_expand(dev, x, m)
        # expand(compact(x, m), compact(x, ~m), m) == x, every stage on the device; the compacted copies are
        # numel-sized, so neither is an empty buffer
        t, f = check_compact(dev, [x], m)
        out = expand(dev, t.view, f.view, place(m, dev))
        assert np.array_equal(_bits(out.get()), _bits(x)), (numel, density)


def _runs(empty_tiles, full_first):
    """``empty_tiles`` empty tiles, one full tile, a ragged random rest -- or the complement."""
    numel = (empty_tiles + 1) * TILE + TILE + 5
    rng = np.random.default_rng(empty_tiles)
    m = np.zeros(numel, dtype=np.bool_)
    m[empty_tiles * TILE:(empty_tiles + 1) * TILE] = True
    m[(empty_tiles + 1) * TILE:] = rng.random(TILE + 5) < 0.5
    return rng.standard_normal(numel, dtype=np.float32), (~m if full_first else m)


@pytest.mark.parametrize("full_first", [False, True])
@pytest.mark.parametrize("empty_tiles", [1, 37, 1024])
def test_long_runs_of_empty_tiles(sq, dev, empty_tiles, full_first):
    x, m = _runs(empty_tiles, full_first)
    check_compact(dev, [x], m)
    check_expand(dev, x, m)


@pytest.mark.parametrize("residue", range(1, 8))
def test_unaligned_mask_source_and_output_pointers(sq, dev, residue):
    """Mask at ``residue`` mod 8; the three sources at 4, 8 and 12 mod 16, the three outputs at 12, 4 and 8."""
    for numel in (9, 2049, 4 * TILE + 1):
        xs, m = _host_case(numel, 0.5)
        check_compact(dev, xs, m, mask_shift=residue, src_shifts=(4, 8, 12), out_shifts=(12, 4, 8))
        check_expand(dev, xs[0], m, mask_shift=residue, out_shift=4 * (residue % 3 + 1))


@pytest.mark.parametrize("numel", ALL_SIZES)
def test_combine_count_is_the_mask_sum(sq, dev, numel):
    """The count svdq_mask_combine returns (its mask output is held by test_hip_mask_ops.py)."""
    for density in DENSITIES:
        stack = np.stack([_host_case(numel, density)[1], _host_case(numel, 0.05)[1]])
        masks = [place(s, dev) for s in stack]
        for code, want in ((0, stack.any(axis=0)), (1, stack.all(axis=0))):       # SVDQ_MASK_UNION, _INTERSECTION
            out, cnt = mask_combine_guarded(sq, masks, code, dev)
            assert np.array_equal(out.get(), want.astype(np.uint8)), (numel, density, code)
            assert int(cnt.get()[0]) == int(want.sum()), (numel, density, code)
