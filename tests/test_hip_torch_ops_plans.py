"""
The plan side of csrc/svdq_torch.cpp: the plan cache (its twelve-field key, LRU order, eviction at 8, one plan per
stream), every refusal that can be raised around a cached plan, task counts from 1 to 32 through compress -> merge ->
diagnostics, 2-D merge weights, and side streams.  The truth is the ctypes route of tests/test_torch_ops.py on the same
tensors, bit for bit (tests/torch_ops_layer.py).

The cache is process-wide and never shrinks, so these tests assert differences and the limit, never absolute sizes; at a
full cache a hit and a miss both leave the size at 8, and the two are told apart by the allocations a call makes (a miss
allocates the new plan's workspace, a hit does not).

No test here captures a graph: the operators build their pointer tables with host-to-device copies and read counts back,
which a capture does not support.
"""
import pytest
import torch

import torch_ops_layer as L
from torch_ops_layer import (Settings, cache_size, deltas, dev, flat, grown, reference, reference_regions, regions, same,
                             same_bits, table)

pytestmark = pytest.mark.gpu
OPS = None


@pytest.fixture(scope="module", autouse=True)
def _ops_loaded():
    global OPS
    import svdq_amd  # noqa: F401
    from svdq_amd import torch_ops
    torch_ops.load()
    OPS = torch.ops.svdq


def _allocations(fn):
    """(result, device allocations the caching allocator served during ``fn``)."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.memory_stats()["allocation.all.allocated"] - before


# ------------------------------------------------------------------------------------------------ 1. the key
class Spec:
    def __init__(self, rows, n=8, st=None, dtype=torch.float32, gram=False, regroup=False, half_values=False, seed=11):
        self.rows, self.n, self.st, self.dtype, self.gram = list(rows), n, st or Settings(), dtype, gram
        self.regroup, self.half_values, self.seed = regroup, half_values, seed

    def vecs(self):
        if self.regroup:      # the SAME 8 tensors as 8 x 1 or 4 x 2
            ts = deltas([self.rows[0]], 8, self.seed)[0]
            v = [ts[i:i + self.n] for i in range(0, 8, self.n)]
        else:
            v = deltas(self.rows, self.n, self.seed)
        if self.half_values or self.dtype is not torch.float32:
            v = [[t.half().float() for t in ts] for ts in v]
        return [[t.to(self.dtype).contiguous() for t in ts] for ts in v]

    def call(self, vecs):
        op = OPS.compress_task_gram if self.gram else OPS.compress
        return op(flat(vecs), self.n, *self.st.args())

    def reference(self, vecs):
        return reference(self.rows, self.n, vecs, self.st, input_dtype=self.dtype, task_gram=self.gram)


def _field(name, i):
    rows = [1, 13 + i, 257, 4097]      # a base key of the field's own: no other test has cached it
    base = Settings()
    return {
        "rows": (Spec(rows), Spec(rows[:3] + [4098])),
        "n_tasks": (Spec([257 + i] * 8, n=1, regroup=True), Spec([257 + i] * 4, n=2, regroup=True)),
        "max_rank": (Spec(rows), Spec(rows, st=base.but(max_rank=1))),
        "bits": (Spec(rows), Spec(rows, st=base.but(bits=8))),
        "stages": (Spec(rows, st=base.but(stages=1)), Spec(rows)),
        "energy": (Spec(rows), Spec(rows, st=base.but(energy=0.95))),
        "center": (Spec(rows), Spec(rows, st=base.but(center=False))),
        "fp16": (Spec(rows), Spec(rows, st=base.but(fp16=False))),
        "input_type": (Spec(rows, half_values=True), Spec(rows, dtype=torch.float16)),
        "task_gram": (Spec(rows), Spec(rows, gram=True)),
    }[name]


FIELDS = ["rows", "n_tasks", "max_rank", "bits", "stages", "energy", "center", "fp16", "input_type", "task_gram"]


@pytest.mark.parametrize("name", FIELDS)
def test_every_key_field_separates_two_plans(name):
    """A, then B (A with one field flipped), then A again: A's two results are bit-identical, B is the ctypes route's
    result at B's settings -- a plan shared across the flip would give B the wrong one -- and B's plan is one more."""
    A, B = _field(name, FIELDS.index(name))
    va, vb = A.vecs(), B.vecs()
    ref_a, ref_b = A.reference(va), B.reference(vb)
    a1 = A.call(va)
    first = regions(ref_a, *a1[:3])
    n0 = cache_size()
    b = B.call(vb)
    n1 = cache_size()
    assert n1 == grown(n0) and n1 <= L.CACHE_MAX, (name, n0, n1)
    a2 = A.call(va)
    assert cache_size() == n1, "A's plan was still there"
    assert same(regions(ref_a, *a2[:3]), first) and same(first, reference_regions(ref_a)), name
    assert same(regions(ref_b, *b[:3]), reference_regions(ref_b)), name
    if B.gram:
        assert same_bits(b[3], ref_b.compress_task_gram())
    # a consumer with the key of a compress that just ran takes that plan: no new one
    if not B.gram and B.dtype is torch.float32:
        w = torch.linspace(0.5, 1.5, B.n, device=dev())
        # (at a full cache the size cannot show it; the allocations do: a first merge that had to make a plan would
        # allocate its workspace, which the second, a certain hit, does not)
        B.call(vb)
        n2 = cache_size()
        merge = lambda: OPS.merge(b[0], b[1], b[2], B.rows, B.n, *B.st.args(), w, [])
        outs, first = _allocations(merge)
        _, second = _allocations(merge)
        assert cache_size() == n2 and first == second, (name, "merge made a plan of its own", first, second)
        buf, offs = ref_b.merge(w.view(1, B.n))
        torch.cuda.synchronize()
        for p, D in enumerate(B.rows):
            assert same_bits(outs[p], buf[offs[p]:offs[p] + D]), (name, p)


# ------------------------------------------------------------------------------------------------ 2. LRU, eviction
def test_lru_order_and_eviction_at_eight():
    st, n = Settings(), 2
    keys = [[13, 300 + i] for i in range(10)]
    vecs = [deltas(k, n, 70 + i) for i, k in enumerate(keys)]

    def call(i):
        return OPS.compress(flat(vecs[i]), n, *st.args())

    outs, clones = {}, {}
    for i in range(8):
        outs[i] = call(i)
        torch.cuda.synchronize()
        clones[i] = [t.clone() for t in outs[i]]
        assert cache_size() <= L.CACHE_MAX
    # the cache now holds exactly keys 0..7 (a full cache) or at least them (a fresh one)
    _, hit = _allocations(lambda: call(7))
    again0, touched = _allocations(lambda: call(0))      # touch key 0 just before the ninth insert
    assert touched == hit, "key 0 was still cached"
    n8 = cache_size()
    out8, miss = _allocations(lambda: call(8))
    assert miss > hit, "a new key allocates its plan's workspace"
    assert cache_size() == grown(n8) <= L.CACHE_MAX
    _, survived = _allocations(lambda: call(0))
    assert survived == hit, "the key touched just before the insert survived it"
    if n8 == L.CACHE_MAX:      # then key 1 was the least recently used one and went
        _, evicted = _allocations(lambda: call(1))
        assert evicted == miss, "the least recently used key was the one dropped"
    call(9)
    assert cache_size() <= L.CACHE_MAX
    for i in range(8):      # ten distinct keys from whatever the cache held: it is full now
        call(i)
        assert cache_size() <= L.CACHE_MAX
    assert cache_size() == L.CACHE_MAX
    torch.cuda.synchronize()
    # what the first calls returned is the caller's: untouched by every later call and by the eviction of their plans
    for i in range(8):
        assert same(outs[i], clones[i]), i
    ref0 = reference(keys[0], n, vecs[0], st)
    assert same(regions(ref0, *call(0)), regions(ref0, *clones[0])) and same(regions(ref0, *again0), regions(ref0, *clones[0]))
    assert same(regions(ref0, *clones[0]), reference_regions(ref0))


# ------------------------------------------------------------------------------------------------ 3. refusals
class Ctx:
    """One compressed store, plain and masked, with everything the consumers take."""

    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.rows, self.n, self.st = [1, 13, 257, 4099], 6, Settings()
        self.vecs = deltas(self.rows, self.n, 23)
        self.flat = flat(self.vecs)
        self.A = self.st.args()
        self.masks = [(torch.rand(D, generator=g) < 0.85) for D in self.rows]
        for m in self.masks:
            m[0] = True
        self.masks = [m.to(dev()) for m in self.masks]
        self.base = [torch.randn(D, generator=g).to(dev()) for D in self.rows]
        self.ft = [[self.base[p] + v for v in vs] for p, vs in enumerate(self.vecs)]
        self.w = torch.tensor([0.3, 0.1, 0.2, 0.15, 0.05, 0.2], device=dev())
        self.compress()

    def compress(self):
        self.small, self.basis, self.mean = OPS.compress(self.flat, self.n, *self.A)
        self.msmall, self.mbasis, self.mmean, self.mrows = OPS.compress_masked(self.flat, self.masks, self.n, *self.A)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def _plan_refusals(c):
    """(name, the refused call, message fragment, the good call of the same key): a TORCH_CHECK_VALUE raised while the
    key's plan is out of the cache."""
    n, A, w, rows = c.n, c.A, c.w, c.rows
    short, dbl = c.mean[:10].contiguous(), c.mean.double()
    bad_base = c.base[:3] + [c.base[3][:5]]
    cpu_mask = c.masks[:3] + [c.masks[3].cpu()]
    good_merge = lambda: OPS.merge(c.small, c.basis, c.mean, rows, n, *A, w, c.base)
    good_mm = lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, c.masks, n, *A, w, c.base)
    good_diag = lambda: [OPS.diagnostics(c.flat, [], c.small, c.basis, c.mean, n, *A, False)]
    good_mdiag = lambda: [OPS.diagnostics(c.flat, c.masks, c.msmall, c.mbasis, c.mmean, n, *A, False)]
    good_dfb = lambda: [OPS.diagnostics_from_base(flat(c.ft), c.base, c.small, c.basis, c.mean, n, *A, False)]
    frag_mean = "mean must be the plan's float32 mean buffer"
    return [
        ("merge: short mean", lambda: OPS.merge(c.small, c.basis, short, rows, n, *A, w, c.base), frag_mean, good_merge),
        ("merge: float64 mean", lambda: OPS.merge(c.small, c.basis, dbl, rows, n, *A, w, c.base), frag_mean, good_merge),
        ("merge: small of another plan", lambda: OPS.merge(c.small[:-8].contiguous(), c.basis, c.mean, rows, n, *A, w, c.base),
         "not the buffers of a plan", good_merge),
        ("merge: strided basis", lambda: OPS.merge(c.small, c.basis[::2], c.mean, rows, n, *A, w, c.base),
         "must be contiguous", good_merge),
        ("merge: base tensor of another size", lambda: OPS.merge(c.small, c.basis, c.mean, rows, n, *A, w, bad_base),
         "base tensor 3 does not match", good_merge),
        ("merge_masked: short mean", lambda: OPS.merge_masked(c.msmall, c.mbasis, short, c.masks, n, *A, w, c.base),
         frag_mean, good_mm),
        ("merge_masked: base tensor of another size",
         lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, c.masks, n, *A, w, bad_base), "base tensor 3 does not match",
         good_mm),
        ("diagnostics: short mean", lambda: OPS.diagnostics(c.flat, [], c.small, c.basis, short, n, *A, False), frag_mean,
         good_diag),
        ("diagnostics: one mask too few",
         lambda: OPS.diagnostics(c.flat, c.masks[:3], c.msmall, c.mbasis, c.mmean, n, *A, False),
         "one combined mask per parameter", good_mdiag),
        ("diagnostics: mask of another size",
         lambda: OPS.diagnostics(c.flat, c.masks[:3] + [c.masks[3][:7]], c.msmall, c.mbasis, c.mmean, n, *A, False),
         "Shape mismatch", good_mdiag),
        ("diagnostics_from_base: short mean",
         lambda: OPS.diagnostics_from_base(flat(c.ft), c.base, c.small, c.basis, short, n, *A, False), frag_mean, good_dfb),
        # the mask walk's one-device check: a CPU mask stands in for the second device
        ("merge_masked: a mask on another device",
         lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, cpu_mask, n, *A, w, c.base),
         "merge_masked: all tensors must live on one device", good_mm),
        ("diagnostics: a mask on another device",
         lambda: OPS.diagnostics(c.flat, cpu_mask, c.msmall, c.mbasis, c.mmean, n, *A, False),
         "diagnostics: all tensors must live on one device", good_mdiag),
    ]


N_PLAN_REFUSALS = 13


@pytest.mark.parametrize("i", range(N_PLAN_REFUSALS))
def test_a_refusal_gives_the_plan_back(ctx, i):
    """A ValueError raised between taking the plan out of the cache and giving it back must not cost the plan: the cache
    is as large after the refusal as before it, the outputs of the good call before are unchanged, and the good call after
    gives the same bits.  (The plan used to be destroyed on this way out and rebuilt, with a synchronisation, by the
    next call.)"""
    refusals = _plan_refusals(ctx)
    assert len(refusals) == N_PLAN_REFUSALS
    name, bad, fragment, good = refusals[i]
    before = good()
    torch.cuda.synchronize()
    clones = [t.clone() for t in before]
    n0 = cache_size()
    with pytest.raises(ValueError, match=fragment):
        bad()
    assert cache_size() == n0, (name, "the refusal dropped the cached plan", n0, cache_size())
    after = good()
    torch.cuda.synchronize()
    assert cache_size() == n0
    assert same(before, clones) and same(after, clones), name


def test_refusals_before_any_plan(ctx):
    """Every other TORCH_CHECK_VALUE of the plan operators: ValueError with its message, the cache untouched and the
    store's buffers unchanged.  A list without a single tensor never reaches the operator (the dispatcher has no device
    to go by), so ``compress([])``'s own message cannot be seen from Python; a CPU tensor among device tensors stands in
    for the second device of the one-device checks."""
    c = ctx
    n, A, w, rows = c.n, c.A, c.w, c.rows
    keep = [t.clone() for t in (c.small, c.basis, c.mean, c.msmall, c.mbasis, c.mmean)]
    cpu_in = c.flat[:-1] + [c.flat[-1].cpu()]
    ragged = c.flat[:-1] + [c.flat[-1][:-1]]
    ftf = flat(c.ft)
    table_ = [
        (lambda: OPS.compress(c.flat, 0, *A), "n_tasks tensors per parameter"),
        (lambda: OPS.compress(c.flat[:-1], n, *A), "n_tasks tensors per parameter"),
        (lambda: OPS.compress(cpu_in, n, *A), "all tensors must live on one device"),
        (lambda: OPS.compress(ragged, n, *A), "task tensors differ in size"),
        (lambda: OPS.compress([c.flat[0]] * 33, 33, *A), "n_tasks must be in"),
        (lambda: OPS.compress(c.flat, n, 1.5, *A[1:]), "Energy threshold"),
        (lambda: OPS.compress(c.flat, n, *A[:4], 9, A[5]), "Low bits"),
        (lambda: OPS.compress(c.flat, n, *A[:5], 0), "RTVQ stages"),
        (lambda: OPS.compress_task_gram(c.flat[:-1], n, *A), "n_tasks tensors per parameter"),
        (lambda: OPS.compress_from_base(ftf, c.base[:3], n, *A), "one base tensor per parameter"),
        (lambda: OPS.compress_from_base(ftf, c.base[:3] + [c.base[3].cpu()], n, *A), "all tensors must live on one device"),
        (lambda: OPS.compress_from_base(ftf, c.base[:3] + [c.base[3][:5]], n, *A), "base and fine-tuned tensors differ"),
        (lambda: OPS.compress_masked(c.flat, c.masks[:3], n, *A), "one combined mask per parameter"),
        (lambda: OPS.compress_gather(c.flat, c.masks[:3], n, *A), "one combined mask per parameter"),
        (lambda: OPS.compress_masked(c.flat, c.masks[:3] + [c.masks[3].cpu()], n, *A), "all tensors must live on one device"),
        (lambda: OPS.compress_gather(c.flat, c.masks[:3] + [c.masks[3][:5]], n, *A), "Shape mismatch"),
        (lambda: OPS.merge(c.small, c.basis, c.mean, [], n, *A, w, []), "Empty delta list"),
        (lambda: OPS.merge(c.small, c.basis, c.mean, rows, n, *A, w, c.base[:2]), "one base tensor per parameter, or none"),
        (lambda: OPS.merge(c.small, c.basis, c.mean, rows, n, *A, w[:5], []), r"weights are \[n_tasks\]"),
        (lambda: OPS.merge(c.small, c.basis, c.mean, rows, n, *A, w.view(1, 1, n), []), r"weights are \[n_tasks\]"),
        (lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, [], n, *A, w, []), "Empty mask list"),
        (lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, c.masks, n, *A, w, c.base[:2]),
         "one base tensor per parameter, or none"),
        (lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, c.masks, n, *A, w[:5], []), r"weights are \[n_tasks\]"),
        (lambda: OPS.diagnostics(c.flat, [], c.small.cpu(), c.basis, c.mean, n, *A, False), "all tensors must live on one device"),
        (lambda: OPS.diagnostics(c.flat[:-1], [], c.small, c.basis, c.mean, n, *A, False), "n_tasks tensors per parameter"),
        (lambda: OPS.diagnostics_from_base(ftf, c.base[:3], c.small, c.basis, c.mean, n, *A, False),
         "one base tensor per parameter"),
        (lambda: OPS.diagnostics_from_base(ftf, c.base[:3] + [c.base[3].cpu()], c.small, c.basis, c.mean, n, *A, False),
         "all tensors must live on one device"),
        (lambda: OPS.diagnostics_from_base(ftf, c.base[:3] + [c.base[3][:5]], c.small, c.basis, c.mean, n, *A, False),
         "base and fine-tuned tensors differ"),
        (lambda: OPS.diagnostics_from_base(ftf, c.base, c.small.cpu(), c.basis, c.mean, n, *A, False),
         "all tensors must live on one device"),
        (lambda: OPS.task_gram(c.flat[:-1], n), "n_tasks tensors per parameter"),
        (lambda: OPS.task_gram(ragged, n), "task tensors differ in size"),
    ]
    n0 = cache_size()
    for k, (bad, fragment) in enumerate(table_):
        with pytest.raises(ValueError, match=fragment):
            bad()
        assert cache_size() == n0, (k, fragment)
    with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
        OPS.compress([], n, *A)
    torch.cuda.synchronize()
    assert cache_size() == n0
    for t, k in zip((c.small, c.basis, c.mean, c.msmall, c.mbasis, c.mmean), keep):
        assert torch.equal(t, k)


# ------------------------------------------------------------------------------------------------ 5. task counts
@pytest.mark.parametrize("n", [1, 2, 8, 9, 16, 17, 20, 32])
def test_task_counts_through_compress_merge_diagnostics(n):
    st = Settings()
    vecs = deltas(L.ROWS, n, 100 + n)
    ref = reference(L.ROWS, n, vecs, st)
    small, basis, mean = OPS.compress(flat(vecs), n, *st.args())
    assert same(regions(ref, small, basis, mean), reference_regions(ref)), n
    w = torch.linspace(0.25, 1.0, n, device=dev()) / n
    outs = OPS.merge(small, basis, mean, L.ROWS, n, *st.args(), w, [])
    buf, offs = ref.merge(w.view(1, n))
    torch.cuda.synchronize()
    for p, D in enumerate(L.ROWS):
        assert same_bits(outs[p], buf[offs[p]:offs[p] + D]), (n, p)
    d6 = OPS.diagnostics(flat(vecs), [], small, basis, mean, n, *st.args(), False)
    want = ref.diagnostics(ref.pointer_table(vecs))
    torch.cuda.synchronize()
    assert same_bits(d6, want), n
    d6 = OPS.diagnostics(flat(vecs), [], small, basis, mean, n, *st.args(), True)
    want = ref.diagnostics(ref.pointer_table(vecs), add_mean=True)
    torch.cuda.synchronize()
    assert same_bits(d6, want), (n, "add_mean")


@pytest.mark.parametrize("with_base", [False, True], ids=["delta", "base"])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
def test_merge_weights_of_several_sets(S, with_base):
    """weights [S, N]: the sets' shares are uniform -- ``CompressPlan.merge`` with ``set_share = 1 / S``; a negative
    weight marks a task that is absent from a set."""
    n, st = 8, Settings()
    g = torch.Generator().manual_seed(40 + S)
    vecs = deltas(L.ROWS, n, 300)
    ref = reference(L.ROWS, n, vecs, st)
    small, basis, mean = OPS.compress(flat(vecs), n, *st.args())
    w = torch.rand(S, n, generator=g) + 0.1
    w[S - 1, 2] = -1.0      # task 2 is not in the last set
    w[0, 5] = -1.0
    w = w.to(dev())
    base = [torch.randn(D, generator=g).to(dev()) for D in L.ROWS] if with_base else []
    outs = OPS.merge(small, basis, mean, L.ROWS, n, *st.args(), w, base)
    share = torch.full((S,), 1.0 / S, dtype=torch.float32, device=dev())
    buf, offs = ref.merge(w, set_share=share if S > 1 else None, base_table=table(base) if with_base else None)
    torch.cuda.synchronize()
    for p, D in enumerate(L.ROWS):
        assert same_bits(outs[p], buf[offs[p]:offs[p] + D]), (S, p)
    if S == 1:      # [1, N] and [N] are the same call
        flat_w = OPS.merge(small, basis, mean, L.ROWS, n, *st.args(), w.view(n), base)
        assert same(flat_w, outs)


def test_merge_refuses_a_ninth_set():
    """include/svdq.h: n_sets <= 8.  The streaming pass refuses a ninth set as unsupported -- on both routes."""
    n, st = 8, Settings()
    vecs = deltas(L.ROWS, n, 300)
    ref = reference(L.ROWS, n, vecs, st)
    small, basis, mean = OPS.compress(flat(vecs), n, *st.args())
    w = torch.full((9, n), 0.125, device=dev())
    n0 = cache_size()
    with pytest.raises(RuntimeError, match="at most 8 sets"):
        OPS.merge(small, basis, mean, L.ROWS, n, *st.args(), w, [])
    assert cache_size() == n0
    with pytest.raises(RuntimeError, match="at most 8 sets"):
        ref.merge(w, set_share=torch.full((9,), 1.0 / 9, device=dev()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. streams
def _stream_ops(c):
    n, A, w = c.n, c.A, c.w
    ftf = flat(c.ft)
    return {
        "compress": lambda: OPS.compress(c.flat, n, *A),
        "compress_task_gram": lambda: OPS.compress_task_gram(c.flat, n, *A),
        "compress_from_base": lambda: OPS.compress_from_base(ftf, c.base, n, *A),
        "compress_masked": lambda: OPS.compress_masked(c.flat, c.masks, n, *A),
        "compress_gather": lambda: OPS.compress_gather(c.flat, c.masks, n, *A),
        "merge": lambda: OPS.merge(c.small, c.basis, c.mean, c.rows, n, *A, w, c.base),
        "merge_masked": lambda: OPS.merge_masked(c.msmall, c.mbasis, c.mmean, c.masks, n, *A, w, c.base),
        "diagnostics": lambda: [OPS.diagnostics(c.flat, [], c.small, c.basis, c.mean, n, *A, False)],
        "diagnostics_masked": lambda: [OPS.diagnostics(c.flat, c.masks, c.msmall, c.mbasis, c.mmean, n, *A, False)],
        "diagnostics_from_base": lambda: [OPS.diagnostics_from_base(ftf, c.base, c.small, c.basis, c.mean, n, *A, False)],
    }


def _written(c, name, out):
    """What a call wrote, comparable bit for bit (the packed buffers of the compress family hold unwritten gaps)."""
    if name.startswith("compress"):
        lay = c.st.plan(c.rows, c.n, gram_only=True)
        return regions(lay, *out[:3]) + [t.cpu() for t in out[3:]]
    return [t.cpu() for t in out]


STREAM_OPS = ["compress", "compress_task_gram", "compress_from_base", "compress_masked", "compress_gather", "merge",
              "merge_masked", "diagnostics", "diagnostics_masked", "diagnostics_from_base"]


@pytest.mark.parametrize("name", STREAM_OPS)
def test_a_side_stream_gets_its_own_plan_and_the_same_bits(ctx, name):
    """The first call on a side stream makes a plan of its own although the default stream's plan of the same shapes and
    settings is cached -- seen in the allocations, which tell a miss (the new plan's workspace) from a hit whatever the
    size of the cache -- and the second call reuses it; both give the default stream's bits."""
    op = _stream_ops(ctx)[name]
    want = _written(ctx, name, op())
    _, hit = _allocations(op)      # the default stream's plan is cached now: what a hit allocates
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    n0 = cache_size()

    def on_side():
        with torch.cuda.stream(side):
            out = op()
        side.synchronize()
        return out

    got, first = _allocations(on_side)
    assert first > hit, (name, "plans are keyed by stream: the side stream's first call makes its own", first, hit)
    assert cache_size() == grown(n0), name
    assert same(_written(ctx, name, got), want), name
    n1 = cache_size()
    got, second = _allocations(on_side)      # and again: the stream's plan is reused
    assert second == hit, (name, "the side stream's plan was reused", second, hit)
    assert cache_size() == n1 and same(_written(ctx, name, got), want), name


def test_two_side_streams_interleaved(ctx):
    """A on s1, B on s2, A on s1, B on s2 -- same shapes, different data: every result is its own reference."""
    c = ctx
    n, A = c.n, c.A
    data = [c.flat, flat(deltas(c.rows, n, 977))]
    want = []
    for d in data:
        sm, ba, me = OPS.compress(d, n, *A)
        outs = OPS.merge(sm, ba, me, c.rows, n, *A, c.w, [])
        want.append(_written(c, "compress", (sm, ba, me)) + [t.cpu() for t in outs])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    got = []
    for rep in range(2):
        for d, s in zip(data, streams):
            with torch.cuda.stream(s):
                sm, ba, me = OPS.compress(d, n, *A)
                got.append((sm, ba, me, OPS.merge(sm, ba, me, c.rows, n, *A, c.w, [])))
    for s in streams:
        s.synchronize()
    for j, (sm, ba, me, outs) in enumerate(got):
        assert same(_written(c, "compress", (sm, ba, me)) + [t.cpu() for t in outs], want[j % 2]), j
