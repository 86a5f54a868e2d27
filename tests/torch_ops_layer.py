"""
Shared pieces of the operator-layer tests (tests/test_hip_torch_ops_plans.py, tests/test_hip_torch_ops_inputs.py).  The
truth of every comparison is the route tests/test_torch_ops.py uses: the same entry point of the C ABI reached through
ctypes (``CompressPlan``, ``MaskSet``, ``_native``) on canonical tensors, bit for bit -- that route is itself held to
fp64 models elsewhere in the suite.
"""
import torch

ROWS = [1, 13, 257, 4097]      # tiny: one row, fewer rows than tasks can be, a thread's second row, several blocks
CACHE_MAX = 8


def dev():
    return torch.device("cuda", 0)


class Settings:
    """The six settings every plan operator takes, in the operators' order."""

    def __init__(self, energy=0.9, max_rank=0, center=True, fp16=True, bits=4, stages=2):
        self.energy, self.max_rank, self.center, self.fp16, self.bits, self.stages = energy, max_rank, center, fp16, bits, stages

    def args(self):
        return (self.energy, self.max_rank, self.center, self.fp16, self.bits, self.stages)

    def but(self, **kw):
        s = Settings(*self.args())
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def plan(self, rows, n_tasks, **kw):
        from svdq_amd.pipeline import CompressPlan
        return CompressPlan(rows, n_tasks, energy_threshold=self.energy, max_rank=self.max_rank or None, center=self.center,
                            fp16=self.fp16, low_bits=self.bits, rtvq_stages=self.stages, device=dev(), **kw)


def deltas(rows, n_tasks, seed):
    """vecs[p][t]: fp32 device tensors, seeded."""
    from oracle import svd_hybrid_oracle as orc
    return [[d.to(dev()) for d in orc.synthetic_deltas(D, n_tasks, seed + 31 * i)] for i, D in enumerate(rows)]


def flat(vecs):
    return [v for vs in vecs for v in vs]


def cache_size():
    return int(torch.ops.svdq.plan_cache_size())


def grown(before):
    """The cache size after one new key: one more, up to the limit (the cache is process-wide and never shrinks, so a
    suite that ran other operator tests first arrives here with a full one)."""
    return min(before + 1, CACHE_MAX)


def regions(plan, small, basis, mean):
    """The bytes a run writes into the packed buffers -- the whole small buffer and per parameter U_high, U_low and the
    mean (the packed buffers also hold never-written alignment gaps) -- as CPU byte tensors; ``plan`` gives the layout."""
    from svdq_amd.pipeline import small_views
    torch.cuda.synchronize()
    sm = small_views(small.cpu().numpy(), plan.layout, plan.P, plan.N, plan.S)
    es = 2 if plan.fp16 else 4
    out = [small.cpu()]
    b = basis.cpu()
    m = mean.cpu() if (plan.center and mean is not None) else None
    for p in range(plan.P):
        rows, k, r = int(sm.rows[p]), int(sm.k[p]), int(sm.r[p])
        base = plan.slab_off[p]
        hb = rows * k * es
        lo = base + (hb + 255) // 256 * 256
        out.append(b[base:base + hb])
        out.append(b[lo:lo + rows * (r - k) * es])
        if m is not None:
            out.append(m[plan.mean_off[p]:plan.mean_off[p] + rows].view(torch.uint8))
    return out


def same_bits(x, y):
    """Bit-for-bit equality of two tensors (NaN == NaN: the degenerate quantizer ranges the golden files pin give NaN
    coefficients, which both routes must then produce alike)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.is_floating_point():
        w = {2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
        x, y = x.contiguous().view(w), y.contiguous().view(w)
    return torch.equal(x, y)


def same(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def reference(rows, n_tasks, vecs, st, input_dtype=torch.float32, task_gram=False):
    """The ctypes route: a CompressPlan with these settings, run on ``vecs``.  Returns the plan (its buffers hold the
    result)."""
    plan = st.plan(rows, n_tasks, input_dtype=input_dtype, task_gram=task_gram)
    plan.run(plan.pointer_table(vecs))
    torch.cuda.synchronize()
    return plan


def reference_regions(plan):
    return regions(plan, plan.small, plan.basis, plan.mean)


def table(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(dev())
