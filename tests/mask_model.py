"""
A numpy model of the mask operators (csrc/svdq_mask.hip; host layer MaskSet in mask_loader.py): what every one of them
has to produce, written with numpy's own selection primitives and nothing from the package under test.  No torch ops,
no GPU.  tests/test_mask_model_cpu.py anchors it on the masks the reference itself produced (tests/golden/masks.npz);
tests/test_hip_mask_ops.py compares the kernels with it, integer for integer.
"""
import numpy as np

STRATEGIES = ("union", "intersection", "majority")
WALK_INV = 1 << 62      # bit 62 of a unit start: the unit takes the CLEARED elements of its mask


def _stack(stack):
    s = np.asarray(stack)
    assert s.dtype == np.bool_ and s.ndim == 2 and s.shape[0] >= 1, (s.dtype, s.shape)
    return s


def votes(stack):
    """Number of masks set at every position: int64 [D]."""
    return _stack(stack).sum(axis=0, dtype=np.int64)


def combine(stack, strategy, votes_needed=None):
    """``stack``: bool [n, D].  union = any, intersection = all, majority = ``2 * votes >= n`` (a tie passes), or
    ``votes >= votes_needed`` when that is given."""
    s = _stack(stack)
    if strategy == "union":
        assert votes_needed is None
        return s.any(axis=0)
    if strategy == "intersection":
        assert votes_needed is None
        return s.all(axis=0)
    if strategy == "majority":
        v = votes(s)
        return 2 * v >= s.shape[0] if votes_needed is None else v >= int(votes_needed)
    raise ValueError(f"Unknown mask strategy: {strategy}")


def majority_threshold(stack, threshold):
    """The reference's rule in its own arithmetic: an fp32 vote count against the Python product ``threshold * n``
    cast to fp32."""
    s = _stack(stack)
    return votes(s).astype(np.float32) >= np.float32(threshold * s.shape[0])


def unpack(stream, bit_off, numel):
    """Elements ``bit_off .. bit_off + numel`` of a numpy.packbits stream, as bool."""
    stream = np.asarray(stream)
    assert stream.dtype == np.uint8 and stream.ndim == 1
    bits = np.unpackbits(stream)[bit_off:bit_off + numel]
    assert bits.size == numel, "the stream is shorter than the parameter it should cover"
    return bits.astype(np.bool_)


def indices(mask):
    """Ascending flat positions of the set and of the cleared elements."""
    m = np.asarray(mask).reshape(-1)
    assert m.dtype == np.bool_
    return np.flatnonzero(m), np.flatnonzero(~m)


def compact(x, mask):
    """``x[mask]`` and ``x[~mask]`` of the flattened arrays."""
    m = np.asarray(mask).reshape(-1)
    x = np.asarray(x).reshape(-1)
    assert m.dtype == np.bool_ and x.size == m.size
    return x[m], x[~m]


def unit_starts(mask, rows, n_units_of_param, unit_rows, inverted):
    """Source position of the first row of each of a parameter's work units: unit j starts at the element of rank
    ``j * unit_rows`` among the selected (``inverted``: the cleared) elements, or at ``numel`` when it lies at or past
    ``rows``, the number of rows the plan processes.  Bit 62 carries the polarity."""
    m = np.asarray(mask).reshape(-1)
    assert m.dtype == np.bool_
    sel = np.flatnonzero(~m if inverted else m)
    tag = WALK_INV if inverted else 0
    r0 = np.arange(n_units_of_param, dtype=np.int64) * int(unit_rows)
    # rows above the true count (a caller whose counts and mask disagree) select nothing either
    live = (r0 < int(rows)) & (r0 < sel.size)
    out = np.full(n_units_of_param, m.size, dtype=np.int64)
    out[live] = sel[r0[live]]
    return out | tag
