"""
fp16 / bf16 task tensors read as they are (svdq_plan_set_input_type): every output -- small artifacts, basis, mean,
task Gram, diagnostics -- must be byte-identical to the same call on the tensors converted to fp32 first, with no fp32
copy of the inputs on the device.  Routes that read fp32 only (the mask walk, mixed dtypes, misaligned views) fall back
to the upcast and must give the same results as well.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HALF = [torch.float16, torch.bfloat16]
N_LIST = [1, 2, 3, 5, 8, 13, 16, 17, 20, 24, 32]
D_LIST = [1, 3, 255, 256, 257, 4096 + 5]
BIG = 4 * 1024 * 1024 + 3          # several work units
SETTINGS = (0.9, 0, 4, 2)          # energy, max_rank (0 = none), bits, stages


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _dev():
    return torch.device("cuda", 0)


def _deltas(D, N, dtype, seed, scale=1.0):
    """N task tensors of D elements in ``dtype``: a rank-3 signal plus noise, with values at the bottom of the dtype's
    range (fp16 subnormals; bf16 values around the fp32 normal / denormal boundary) planted at fixed positions."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = _dev()
    r = min(3, N)
    A = torch.randn(D, r, generator=g, device=dev) @ torch.randn(r, N, generator=g, device=dev)
    A = scale * (A + 0.05 * torch.randn(D, N, generator=g, device=dev))
    out = []
    for t in range(N):
        x = A[:, t].to(dtype).contiguous()
        if dtype is torch.float16:
            tiny = torch.tensor([2.0 ** -24, -3 * 2.0 ** -20, 2.0 ** -15, 6.0e-5], device=dev)
        else:
            tiny = torch.tensor([1.0e-38, -2.0e-39, 1.2e-38, 9.0e-41], device=dev)
        pos = torch.arange(t % 7, D, 11, device=dev)[: 4 * max(1, D // 44)] if t % 7 < D else None
        if pos is not None and pos.numel():
            x[pos] = tiny[torch.arange(pos.numel(), device=dev) % 4].to(dtype)
        out.append(x)
    return out


def _regions(sq, rows_upper, N, center, fp16, small, basis, mean):
    """The bytes a run writes: the whole small buffer, and per parameter U_high, U_low and the mean (the packed
    buffers also hold never-written alignment gaps)."""
    lay = sq.pipeline.CompressPlan(rows_upper, N, center=center, fp16=fp16, gram_only=True, device=_dev())
    L = lay.layout
    P = len(rows_upper)
    sm = small.cpu()
    k = sm[L.k_off:L.k_off + 4 * P].view(torch.int32).tolist()
    r = sm[L.r_off:L.r_off + 4 * P].view(torch.int32).tolist()
    rows = sm[L.rows_off:L.rows_off + 8 * P].view(torch.int64).tolist()
    es = 2 if fp16 else 4
    out = [small]
    for p in range(P):
        s, hi = lay.slab_off[p], rows[p] * k[p] * es
        out.append(basis[s:s + hi])
        lo = s + (hi + 255) // 256 * 256
        out.append(basis[lo:lo + rows[p] * (r[p] - k[p]) * es])
        if center:
            out.append(mean[lay.mean_off[p]:lay.mean_off[p] + rows[p]].view(torch.uint8))
    lay.close()
    return out


def _same_bytes(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.numel() == y.numel() and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"region {i} differs"


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", N_LIST)
def test_compress_bit_identical(sq, N, dtype):
    energy, max_rank, bits, stages = SETTINGS
    for center, fp16 in [(True, True), (True, False), (False, True), (False, False)]:
        Ds = D_LIST + ([BIG] if (center and fp16) else [])
        half = [v for i, D in enumerate(Ds) for v in _deltas(D, N, dtype, 1000 * N + i)]
        full = [v.float() for v in half]
        a = torch.ops.svdq.compress(half, N, energy, max_rank, center, fp16, bits, stages)
        b = torch.ops.svdq.compress(full, N, energy, max_rank, center, fp16, bits, stages)
        _same_bytes(_regions(sq, Ds, N, center, fp16, *a), _regions(sq, Ds, N, center, fp16, *b))
        if center and fp16:
            # task Gram (fp64, exact equality) and the plain diagnostics against the same artifacts
            assert torch.equal(torch.ops.svdq.task_gram(half, N), torch.ops.svdq.task_gram(full, N))
            d_half = torch.ops.svdq.diagnostics(half, [], *b, N, energy, max_rank, center, fp16, bits, stages, False)
            d_full = torch.ops.svdq.diagnostics(full, [], *b, N, energy, max_rank, center, fp16, bits, stages, False)
            _same_bytes([d_half], [d_full])      # byte equality: tasks without signal give NaN relative errors


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [1, 3, 8, 13, 17, 20, 32])
def test_compress_from_base_bit_identical(sq, N, dtype):
    energy, max_rank, bits, stages = SETTINGS
    Ds = D_LIST + ([BIG] if N == 8 else [])
    base = [_deltas(D, 1, dtype, 77 + i, scale=3.0)[0] for i, D in enumerate(Ds)]
    ft = [(b.float() + d.float()).to(dtype) for i, (b, D) in enumerate(zip(base, Ds))
          for d in _deltas(D, N, dtype, 500 * N + i)]
    for center, fp16 in [(True, True), (False, False)]:
        a = torch.ops.svdq.compress_from_base(ft, base, N, energy, max_rank, center, fp16, bits, stages)
        b = torch.ops.svdq.compress_from_base([f.float() for f in ft], [x.float() for x in base], N, energy,
                                              max_rank, center, fp16, bits, stages)
        _same_bytes(_regions(sq, Ds, N, center, fp16, *a), _regions(sq, Ds, N, center, fp16, *b))


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [5, 20])
def test_compress_gather_bit_identical(sq, N, dtype):
    energy, max_rank, bits, stages = SETTINGS
    Ds = [257, 4096 + 5, 70001]
    g = torch.Generator(device="cuda").manual_seed(N)
    masks = [torch.rand(D, generator=g, device=_dev()) < 0.2 for D in Ds]
    half = [v for i, D in enumerate(Ds) for v in _deltas(D, N, dtype, 300 + i)]
    for center, fp16 in [(True, True), (False, False)]:
        a = torch.ops.svdq.compress_gather(half, masks, N, energy, max_rank, center, fp16, bits, stages)
        b = torch.ops.svdq.compress_gather([v.float() for v in half], masks, N, energy, max_rank, center, fp16, bits,
                                           stages)
        assert torch.equal(a[3], b[3])
        _same_bytes(_regions(sq, Ds, N, center, fp16, *a[:3]), _regions(sq, Ds, N, center, fp16, *b[:3]))


def _config(sq, **kw):
    cfg = sq.config.SVDHybridConfig()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _model(N, dtype, with_base, seed):
    """{task: {param: tensor}}: two unmasked parameters and two with sparse masks (index lists); fine-tuned weights and
    a base state when ``with_base``."""
    shapes = {"a.weight": (64, 96), "a.bias": (257,), "m.weight": (300, 40), "m2.weight": (4101,)}
    tasks = [f"t{i}" for i in range(N)]
    tv = {t: {} for t in tasks}
    base = {}
    for j, (name, s) in enumerate(shapes.items()):
        D = int(np.prod(s))
        ds = _deltas(D, N, dtype, seed + j)
        b = _deltas(D, 1, dtype, seed + 50 + j, scale=2.0)[0] if with_base else None
        if with_base:
            base[name] = b.view(s)
        for i, t in enumerate(tasks):
            x = (b.float() + ds[i].float()).to(dtype) if with_base else ds[i]
            tv[t][name] = x.view(s)
    g = torch.Generator(device="cuda").manual_seed(seed)
    masks = {n: torch.rand(shapes[n], generator=g, device=_dev()) < 0.25 for n in ("m.weight", "m2.weight")}
    return tv, (base if with_base else None), masks


def _plans(bases):
    out = {}
    for name, b in bases.items():
        for region in ("masked", "noise"):
            x = b.get(region)
            if x is not None and getattr(x, "_batch", None) is not None:
                batch = x._batch[0]
                out[tuple(batch.entries)] = batch
    return out


def _compare_batches(ba, bb):
    pa, pb = _plans(ba), _plans(bb)
    assert sorted(pa) == sorted(pb)
    for key in pa:
        A, B = pa[key], pb[key]
        assert torch.equal(A.plan.small, B.plan.small), key
        for i in range(len(key)):
            k, r, rows = int(A.small.k[i]), int(A.small.r[i]), int(A.small.rows[i])
            for x, y in zip(A.plan.basis_tensors(i, k, r, rows), B.plan.basis_tensors(i, k, r, rows)):
                if x is not None:
                    assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x,
                                       y.view(torch.uint8) if y.dtype != torch.uint8 else y), (key, i)
    return pa


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
@pytest.mark.parametrize("N", [5, 20])
@pytest.mark.parametrize("with_base", [False, True], ids=["deltas", "from_base"])
def test_driver_routes_bit_identical(sq, N, dtype, with_base):
    """plain, gather, from-base and gather-from-base through driver.build_bases, native against upcast first."""
    tv, base, masks = _model(N, dtype, with_base, 40 + N)
    cfg = _config(sq, svd_include_noise=True)
    up = {t: {n: v.float() for n, v in d.items()} for t, d in tv.items()}
    upb = {n: v.float() for n, v in base.items()} if base is not None else None
    ba = sq.driver.build_bases(tv, masks, cfg, _dev(), base_state=base)
    bb = sq.driver.build_bases(up, masks, cfg, _dev(), base_state=upb)
    plans = _compare_batches(ba, bb)
    modes = {b.mode: b.plan.input_dtype for b in plans.values()}
    assert modes.get("plain") is dtype and modes.get("gather") is dtype, modes


# ------------------------------------------------------------------------------------------------ no fp32 copies
def _plan_bytes(plan):
    s = plan.sizes
    return int(s.workspace_bytes) + (int(s.basis_bytes) + 255) // 256 * 256 + int(s.mean_floats) * 4 + int(s.small_bytes)


@pytest.mark.parametrize("route", ["driver", "from_checkpoints", "op"])
def test_no_fp32_copy(sq, route):
    N, dev = 8, _dev()
    shapes = {"w1": (1024, 1024), "w2": (2048, 512)}
    tv = {f"t{i}": {n: _deltas(int(np.prod(s)), 1, torch.bfloat16, 10 * i + j)[0].view(s)
                    for j, (n, s) in enumerate(shapes.items())} for i in range(N)}
    base = {n: _deltas(int(np.prod(s)), 1, torch.bfloat16, 99 + j)[0].view(s) for j, (n, s) in enumerate(shapes.items())}
    cfg = _config(sq)
    rows = [int(np.prod(s)) for s in shapes.values()]
    ref = sq.pipeline.CompressPlan(rows, N, center=cfg.svd_center, fp16=cfg.svd_fp16, device=dev, gram_only=True)
    budget = _plan_bytes(ref) + 1024 * 1024
    ref.close()
    input_bytes = sum(v.numel() * 2 for d in tv.values() for v in d.values())
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    if route == "driver":
        bases, _ = sq.driver.run_basis_and_compress(tv, None, cfg, dev)
    elif route == "from_checkpoints":
        bases, _ = sq.driver.run_basis_and_compress_from_checkpoints(base, tv, cfg, dev)
    else:
        flat = [tv[t][n] for n in shapes for t in tv]
        out = torch.ops.svdq.compress(flat, N, cfg.svd_energy_threshold, 0, cfg.svd_center, cfg.svd_fp16,
                                      cfg.svd_low_bits, cfg.svd_rtvq_stages)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - before
    assert extra <= budget, f"peak extra {extra / 2**20:.1f} MiB > plan buffers + 1 MiB = {budget / 2**20:.1f} MiB " \
                            f"(inputs {input_bytes / 2**20:.0f} MiB)"
    if route != "op":
        assert all(b.plan.input_dtype is torch.bfloat16 for b in _plans(bases).values())


# ------------------------------------------------------------------------------------------------ ABI
def test_set_input_type_abi(sq):
    from ctypes import c_void_p
    nat, dev = sq._native, _dev()
    lib = nat.lib()
    plan = sq.pipeline.CompressPlan([4096], 4, device=dev)
    h = plan._h
    for bad in (-1, 3, 7):
        assert lib.svdq_plan_set_input_type(h, bad) == nat.SVDQ_EINVAL
        assert "input type" in nat.last_error()
    assert lib.svdq_plan_set_input_type(None, 1) == nat.SVDQ_EINVAL
    for ok in (nat.SVDQ_INPUT_F16, nat.SVDQ_INPUT_F32, nat.SVDQ_INPUT_BF16):
        assert lib.svdq_plan_set_input_type(h, ok) == nat.SVDQ_OK
    # a bf16 plan: every entry point whose kernels read task tensors as fp32 only refuses, naming itself
    junk = torch.zeros(4096, dtype=torch.int64, device=dev)
    p = c_void_p(junk.data_ptr())
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = {
        "svdq_compress_masked": lambda: lib.svdq_compress_masked(h, p, p, p, p, p, p, p, p, st),
        "svdq_compress_masked_from_base": lambda: lib.svdq_compress_masked_from_base(h, p, p, p, p, p, p, p, p, p, st),
        "svdq_diagnostics_masked": lambda: lib.svdq_diagnostics_masked(h, p, p, p, p, p, p, p, 0, p, p, st),
        "svdq_ingest": lambda: lib.svdq_ingest(h, p, p, p, None, st),
        "svdq_tvq_quantize": lambda: lib.svdq_tvq_quantize(h, p, 0, 8, p, p, p, p, 0, st),
        "svdq_tvq_dequantize": lambda: lib.svdq_tvq_dequantize(h, p, 0, p, p, None, p, st),
    }
    for name, call in calls.items():
        assert call() == nat.SVDQ_EUNSUPPORTED, name
        assert name in nat.last_error() and "SVDQ_INPUT_BF16" in nat.last_error(), nat.last_error()
    torch.cuda.synchronize()
    plan.close()


# ------------------------------------------------------------------------------------------------ fallbacks
def _op(vecs, N, center=True, fp16=True):
    energy, max_rank, bits, stages = SETTINGS
    return torch.ops.svdq.compress(vecs, N, energy, max_rank, center, fp16, bits, stages)


def test_mixed_dtypes_upcast(sq):
    N, Ds = 5, [257, 4101]
    vecs = []
    for i, D in enumerate(Ds):
        vs = _deltas(D, N, torch.bfloat16, 60 + i)
        vecs += [v if t < 3 else v.float() for t, v in enumerate(vs)]
    a = _op(vecs, N)
    b = _op([v.float() for v in vecs], N)
    _same_bytes(_regions(sq, Ds, N, True, True, *a), _regions(sq, Ds, N, True, True, *b))
    tv = {f"t{t}": {"p": vecs[t]} for t in range(N)}
    bases = sq.driver.build_bases(tv, None, _config(sq), _dev())
    assert all(b.plan.input_dtype is torch.float32 for b in _plans(bases).values())
    ref = sq.driver.build_bases({t: {n: v.float() for n, v in d.items()} for t, d in tv.items()}, None, _config(sq),
                                _dev())
    _compare_batches(bases, ref)


@pytest.mark.parametrize("dtype", HALF, ids=["f16", "bf16"])
def test_misaligned_half_view(sq, dtype):
    N, D = 3, 4101
    store = [_deltas(D + 1, 1, dtype, 80 + t)[0] for t in range(N)]
    views = [s[1:] for s in store]                    # storage offset 1: 2 bytes past an aligned start
    assert all(v.data_ptr() % 8 for v in views)
    a = _op(views, N)
    b = _op([v.float() for v in views], N)
    _same_bytes(_regions(sq, [D], N, True, True, *a), _regions(sq, [D], N, True, True, *b))
    tv = {f"t{t}": {"p": views[t]} for t in range(N)}
    ba = sq.driver.build_bases(tv, None, _config(sq), _dev())
    bb = sq.driver.build_bases({t: {"p": d["p"].float()} for t, d in tv.items()}, None, _config(sq), _dev())
    plans = _compare_batches(ba, bb)
    assert all(b.plan.input_dtype is dtype for b in plans.values())


def test_dense_mask_walk_upcasts(sq):
    N = 5
    tv, _, _ = _model(N, torch.bfloat16, False, 7)
    g = torch.Generator(device="cuda").manual_seed(3)
    masks = {n: torch.rand(tv["t0"][n].shape, generator=g, device=_dev()) < 0.8 for n in ("m.weight", "m2.weight")}
    cfg = _config(sq)
    ba = sq.driver.build_bases(tv, masks, cfg, _dev())
    bb = sq.driver.build_bases({t: {n: v.float() for n, v in d.items()} for t, d in tv.items()}, masks, cfg, _dev())
    plans = _compare_batches(ba, bb)
    modes = {b.mode: b.plan.input_dtype for b in plans.values()}
    assert modes.get("walk") is torch.float32 and modes.get("plain") is torch.bfloat16, modes


# ------------------------------------------------------------------------------------------------ CLI
def _load_tree(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _assert_same_tree(a, b, where):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape, where
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), where
    elif isinstance(a, dict):
        assert sorted(a.keys(), key=str) == sorted(b.keys(), key=str), where
        for k in a:
            _assert_same_tree(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same_tree(x, y, f"{where}[{i}]")
    elif isinstance(a, float) and a != a:
        assert isinstance(b, float) and b != b, where       # NaN in both
    else:
        assert a == b, where


@pytest.mark.parametrize("route", ["from_checkpoints", "task_vectors"])
def test_cli_fp16_checkpoints(sq, tmp_path, route):
    """--no-eval-reconstruction: fine-tuned and base tensors go to the passes as they are (svdq_compress_from_base on
    fp16 inputs); the default run forms the task vectors first (svdq_ingest, fp32)."""
    tasks = ["Cars", "DTD", "EuroSAT", "MNIST"]
    g = torch.Generator().manual_seed(5)
    shapes = {"blk.attn.weight": (96, 64), "blk.attn.bias": (96,), "blk.mlp.weight": (128, 64), "ln.weight": (64,)}
    base = {k: torch.randn(s, generator=g).half() for k, s in shapes.items()}
    fts = {t: {k: (base[k].float() + 0.05 * torch.randn(s, generator=g)).half() for k, s in shapes.items()}
           for t in tasks}
    arts = {}
    for label, cast in (("half", lambda x: x), ("float", lambda x: x.float())):
        root = tmp_path / label
        (root / "ckpt").mkdir(parents=True)
        torch.save({k: cast(v) for k, v in base.items()}, root / "base.pt")
        for t in tasks:
            torch.save({k: cast(v) for k, v in fts[t].items()}, root / "ckpt" / f"{t}.pt")
        argv = ["--tasks", *tasks, "--checkpoint-dir", str(root / "ckpt"), "--base-model-path", str(root / "base.pt"),
                "--energy-threshold", "0.9", "--low-bits", "4", "--rtvq-stages", "2", "--weighting", "uniform",
                "--store-artifacts", "--output-dir", str(root / "out"), "--artifact-dir", str(root / "art")]
        if route == "from_checkpoints":
            argv.append("--no-eval-reconstruction")
        sq.cli.main(argv)
        arts[label] = root / "art"
    for sub in ("basis", "coeffs"):
        names = sorted(os.listdir(arts["half"] / sub))
        assert names and names == sorted(os.listdir(arts["float"] / sub))
        for n in names:
            _assert_same_tree(_load_tree(arts["half"] / sub / n), _load_tree(arts["float"] / sub / n), f"{sub}/{n}")
