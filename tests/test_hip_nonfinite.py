"""
Non-finite task deltas on the GPU (include/svdq.h, svdq_eig_rank_select: the one statement of the contract).

The reference stops on a delta that holds NaN or +-Inf (torch.linalg.svd raises in compute_svd, basis.py:216-249).
Here the eigen stage flags such a parameter with a NaN energy in the small buffer, ``CompressPlan.fetch_small`` raises
``NonFiniteInput`` and the dictionary API a RuntimeError that names the parameter and its region.  NaN and Inf are
ordinary data for the kernels: no test here provokes a fault, and every run ends.

Without the feature every "raises" case fails: the parent returns a zero basis, sigma = 0 and k = 1 for such input.
"""
import json
import os

import numpy as np
import pytest
import torch

from test_nonfinite_cpu import small_layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = [1, 3, 257, 4101, 4 * 2 ** 20 + 3]
NAMES = ["layer0.w_d1", "layer1.w_d3", "layer2.w_d257", "layer3.w_d4101", "layer4.w_dbig"]
TASK_COUNTS = [1, 3, 8, 16, 17, 20, 32]
VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
WORDING = "input matrix contained non-finite values"      # torch.linalg.svd's, what the reference's run ends with


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import svd_hybrid_oracle
    return svd_hybrid_oracle


def _cfg(sq, **kw):
    base = dict(svd_energy_threshold=0.9, svd_max_rank=64, svd_center=True, svd_fp16=True, svd_low_bits=4,
                svd_rtvq_stages=2, svd_include_noise=False, svd_min_mask_size=10)
    base.update(kw)
    return sq.SVDHybridConfig(**base)


def _positions(D):
    """Row 0, a row inside the last (partial) 256-row block, the last row."""
    last_block = (D - 1) // 256 * 256
    return sorted({0, (last_block + D - 1) // 2, D - 1})


def _ragged(N, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [[(0.01 * torch.randn(D, generator=g, device="cuda")).to(dtype) for _ in range(N)] for D in ROWS]


def _host_small(sq, plan):
    """The typed views fetch_small returns, without its checks."""
    host = plan.small.cpu().numpy()
    L, P, N = plan.layout, plan.P, plan.N
    f = lambda off, dt, n: host[off:off + n * np.dtype(dt).itemsize].view(dt)      # noqa: E731
    return {"sigma": f(L.sigma_off, np.float32, P * N).reshape(P, N), "k": f(L.k_off, np.int32, P),
            "r": f(L.r_off, np.int32, P), "energy": f(L.energy_off, np.float32, P), "rows": f(L.rows_off, np.int64, P)}


def _names_in(msg):
    return [n for n in NAMES if repr(n) in msg]


# ------------------------------------------------------------------------------------------- ragged plans
@pytest.mark.parametrize("N", TASK_COUNTS)
def test_planted_value_raises_and_names_the_parameter(sq, N):
    vectors = _ragged(N, 40 + N)
    tasks = [f"task{t:02d}" for t in range(N)]
    task_vectors = {t: {n: vectors[p][ti] for p, n in enumerate(NAMES)} for ti, t in enumerate(tasks)}
    cfg = _cfg(sq)
    plan = sq.pipeline.CompressPlan(ROWS, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4,
                                    rtvq_stages=2, device="cuda")
    L = small_layout(sq, len(ROWS), N, 2)      # the arithmetic the CPU tests build their buffers with
    assert all(getattr(L, f) == getattr(plan.layout, f) for f, _ in L._fields_)
    table = plan.pointer_table(vectors)
    n_cases = 0
    for p, D in enumerate(ROWS):
        for pi, row in enumerate(_positions(D)):
            for vi, (what, val) in enumerate(VALUES.items()):
                t = (p + pi + vi) % N
                keep = vectors[p][t][row].clone()
                vectors[p][t][row] = val
                try:
                    case = (N, NAMES[p], row, what, t)
                    # the plan itself: one parameter flagged, the others healthy, indices in range
                    plan.run(table)
                    assert sq.pipeline.nonfinite_parameters(plan.small, plan.layout, plan.P) == [p], case
                    sm = _host_small(sq, plan)
                    assert np.isnan(sm["sigma"][p]).all() and np.isnan(sm["energy"][p]), case
                    healthy = [q for q in range(len(ROWS)) if q != p]
                    assert np.isfinite(sm["energy"][healthy]).all() and np.isfinite(sm["sigma"][healthy]).all(), case
                    r = np.minimum(np.array(ROWS), N)
                    assert (sm["r"] == r).all() and (sm["rows"] == np.array(ROWS)).all(), case
                    assert (sm["k"] >= np.minimum(1, r)).all() and (sm["k"] <= r).all(), case
                    with pytest.raises(sq.pipeline.NonFiniteInput) as ei:
                        plan.fetch_small()
                    assert ei.value.indices == [p], case
                    # the dictionary API: a RuntimeError that names this parameter and no healthy one
                    with pytest.raises(RuntimeError, match=WORDING) as ei:
                        sq.driver.run_basis_and_compress(task_vectors, None, cfg, "cuda")
                    assert _names_in(str(ei.value)) == [NAMES[p]], (case, str(ei.value))
                    n_cases += 1
                finally:
                    vectors[p][t][row] = keep
    assert n_cases == 3 * sum(len(_positions(D)) for D in ROWS)
    # the same buffers, clean inputs: nothing stale
    plan.run(table)
    assert sq.pipeline.nonfinite_parameters(plan.small, plan.layout, plan.P) == []
    sm = plan.fetch_small()
    assert np.isfinite(sm.energy).all() and np.isfinite(sm.sigma).all()
    bases, comp = sq.driver.run_basis_and_compress(task_vectors, None, cfg, "cuda")
    assert sorted(bases) == sorted(NAMES) == sorted(comp)


@pytest.mark.parametrize("N", [3, 8, 20])
@pytest.mark.parametrize("center", [True, False])
def test_inf_in_two_tasks_at_one_row(sq, N, center):
    """Centred, the mean of that row is +Inf and every centred value NaN; uncentred, the Gram holds +Inf."""
    vectors = _ragged(N, 90 + N)
    tasks = [f"task{t:02d}" for t in range(N)]
    p, row = 3, 2049
    vectors[p][0][row] = float("inf")
    vectors[p][N - 1][row] = float("inf")
    task_vectors = {t: {n: vectors[q][ti] for q, n in enumerate(NAMES)} for ti, t in enumerate(tasks)}
    with pytest.raises(RuntimeError, match=WORDING) as ei:
        sq.driver.run_basis_and_compress(task_vectors, None, _cfg(sq, svd_center=center), "cuda")
    assert _names_in(str(ei.value)) == [NAMES[p]]


@pytest.mark.parametrize("N", [8, 20])
@pytest.mark.parametrize("both", [False, True])
def test_from_checkpoints(sq, N, both):
    """Base +Inf under a finite fine-tuned tensor (delta -Inf), and both +Inf at one row (delta NaN)."""
    deltas = _ragged(N, 120 + N)
    g = torch.Generator(device="cuda").manual_seed(7)
    base = {n: torch.randn(D, generator=g, device="cuda") for n, D in zip(NAMES, ROWS)}
    tasks = [f"task{t:02d}" for t in range(N)]
    fine = {t: {n: base[n] + deltas[p][ti] for p, n in enumerate(NAMES)} for ti, t in enumerate(tasks)}
    cfg = _cfg(sq)
    bases, _ = sq.driver.run_basis_and_compress_from_checkpoints(base, fine, cfg, "cuda")       # clean: no raise
    assert sorted(bases) == sorted(NAMES)
    p, row = 2, 256
    base[NAMES[p]][row] = float("inf")
    if both:
        fine[tasks[1]][NAMES[p]][row] = float("inf")
    with pytest.raises(RuntimeError, match=WORDING) as ei:
        sq.driver.run_basis_and_compress_from_checkpoints(base, fine, cfg, "cuda")
    assert _names_in(str(ei.value)) == [NAMES[p]]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N", [8, 20])
def test_half_inputs_read_natively(sq, dtype, N):
    vectors = _ragged(N, 150 + N, dtype)
    tasks = [f"task{t:02d}" for t in range(N)]
    task_vectors = {t: {n: vectors[p][ti] for p, n in enumerate(NAMES)} for ti, t in enumerate(tasks)}
    assert sq.pipeline.native_input_dtype(v for vs in vectors for v in vs) is dtype
    cfg = _cfg(sq)
    bases, _ = sq.driver.run_basis_and_compress(task_vectors, None, cfg, "cuda")
    assert sorted(bases) == sorted(NAMES)
    for p, (what, val) in zip((1, 3, 4), VALUES.items()):
        row = _positions(ROWS[p])[1]
        keep = vectors[p][N - 1][row].clone()
        vectors[p][N - 1][row] = val                      # the NaN / Inf of that dtype
        assert not torch.isfinite(vectors[p][N - 1][row])
        with pytest.raises(RuntimeError, match=WORDING) as ei:
            sq.driver.run_basis_and_compress(task_vectors, None, cfg, "cuda")
        assert _names_in(str(ei.value)) == [NAMES[p]], (what, str(ei.value))
        vectors[p][N - 1][row] = keep


# ------------------------------------------------------------------------------------------- masked regions
def _masked_setup(N, density, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shapes = {"blk.attn.weight": (64, 96), "blk.mlp.weight": (48, 64), "blk.attn.bias": (96,)}
    tasks = [f"task{t:02d}" for t in range(N)]
    tv = {t: {n: 0.01 * torch.randn(s, generator=g, device="cuda") for n, s in shapes.items()} for t in tasks}
    masks = {n: torch.rand(s, generator=g, device="cuda") < density for n, s in shapes.items() if n.endswith("weight")}
    return tasks, tv, masks


def _artifact_bytes(bases, comp):
    """Every artifact of the run as host arrays: the small buffers whole, the basis and mean tensors per region."""
    out, seen = {}, set()
    for n in sorted(bases):
        for region in ("masked", "noise"):
            b = bases[n][region]
            if b is None:
                continue
            batch, _ = b._batch
            if id(batch) not in seen:
                seen.add(id(batch))
                out[f"small{len(seen)}"] = batch.plan.small.cpu().numpy().copy()
            for key in ("U_high", "U_low", "mean", "singular_values"):
                out[f"{n}/{region}/{key}"] = b[key].cpu().contiguous().view(torch.uint8).numpy().copy()
        for t, art in comp[n].items():
            for region in ("masked", "unmasked"):
                if art[region] is not None:
                    out[f"{n}/{t}/{region}/c_high"] = art[region]["c_high_fp16"].view(torch.uint8).numpy().copy()
    return out


# dense mask: the signal region is walked (svdq_compress_masked), the noise region gathered; sparse mask: the reverse
@pytest.mark.parametrize("route,density", [("walk", 0.8), ("gather", 0.2)])
def test_masked_regions(sq, route, density):
    N = 8
    tasks, tv, masks = _masked_setup(N, density, 11)
    name = "blk.attn.weight"
    assert (float(masks[name].float().mean()) >= sq.driver.WALK_MIN_DENSITY) == (route == "walk")
    flat_mask = masks[name].view(-1)
    cleared = int(torch.nonzero(~flat_mask)[5])
    setpos = int(torch.nonzero(flat_mask)[5])
    victim = tv[tasks[2]][name].view(-1)

    # a NaN at a cleared position, signal region only: the reference never sees it -- no raise, and every artifact
    # byte is that of the run with a 0 there
    victim[cleared] = 0.0
    want = _artifact_bytes(*sq.driver.run_basis_and_compress(tv, masks, _cfg(sq), "cuda"))
    victim[cleared] = float("nan")
    got = _artifact_bytes(*sq.driver.run_basis_and_compress(tv, masks, _cfg(sq), "cuda"))
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    # with the noise region it is input: raises and names the noise region, not the signal region
    with pytest.raises(RuntimeError, match=WORDING) as ei:
        sq.driver.run_basis_and_compress(tv, masks, _cfg(sq, svd_include_noise=True), "cuda")
    msg = str(ei.value)
    assert f"{name!r} [noise]" in msg and f"{name!r} [masked]" not in msg and "blk.mlp.weight" not in msg, msg
    victim[cleared] = 0.0

    # a NaN at a set position: the signal region, with or without the noise region beside it
    victim[setpos] = float("nan")
    for include_noise in (False, True):
        with pytest.raises(RuntimeError, match=WORDING) as ei:
            sq.driver.run_basis_and_compress(tv, masks, _cfg(sq, svd_include_noise=include_noise), "cuda")
        msg = str(ei.value)
        assert f"{name!r} [masked]" in msg and f"{name!r} [noise]" not in msg and "blk.mlp.weight" not in msg, msg


@pytest.mark.parametrize("include_noise", [False, True])
def test_gated_region_is_never_read(sq, include_noise):
    """A mask of 9 set elements is below svd_min_mask_size = 10: the reference skips the parameter (cli.py:332, :343)
    and never sees the NaN at a set position, nor -- the noise region is gated on the signal count -- at a cleared one."""
    N = 4
    tasks, tv, masks = _masked_setup(N, 0.8, 13)
    name = "blk.attn.weight"
    m = torch.zeros(64 * 96, dtype=torch.bool, device="cuda")
    m[torch.arange(9, device="cuda") * 601 + 17] = True
    masks[name] = m.view(64, 96)
    assert int(masks[name].sum()) == 9
    tv[tasks[1]][name].view(-1)[17] = float("nan")           # a set position
    tv[tasks[2]][name].view(-1)[18] = float("inf")           # a cleared one
    bases, comp = sq.driver.run_basis_and_compress(tv, masks, _cfg(sq, svd_include_noise=include_noise), "cuda")
    assert name not in bases and name not in comp
    assert sorted(bases) == ["blk.attn.bias", "blk.mlp.weight"]


# ------------------------------------------------------------------------------------------- no false alarms
def _s64(deltas, center):
    """fp64 singular values of exactly the matrix the reference factorises (fp32 stack, fp32 centring)."""
    T = torch.stack([d.float().cpu() for d in deltas], dim=1)
    if center:
        T = T - T.mean(dim=1, keepdim=True)
    return torch.linalg.svdvals(T.double()).numpy()


def test_healthy_edge_inputs_do_not_raise(sq):
    dev = "cuda"
    kw = dict(energy_threshold=0.9, max_rank=None, center=True, fp16=True, low_bits=4, rtvq_stages=2, device=dev)
    for N in (8, 20):
        # all-zero deltas
        _, sm = sq.compress_batch([[torch.zeros(D, device=dev) for _ in range(N)] for D in ROWS[:4]], **kw)
        assert np.isfinite(sm.energy).all() and (sm.sigma == 0).all()
        # D < N
        g = torch.Generator(device=dev).manual_seed(N)
        _, sm = sq.compress_batch([[torch.randn(3, generator=g, device=dev) for _ in range(N)]], **kw)
        assert np.isfinite(sm.energy).all() and int(sm.r[0]) == 3
        # fp16 subnormals, read natively
        sub = [[(torch.randint(-1023, 1024, (D,), generator=g, device=dev).float() * 2.0 ** -24).half()
                for _ in range(N)] for D in (257, 4101)]
        assert all(float(v.float().abs().max()) < 6.2e-5 for vs in sub for v in vs)
        _, sm = sq.compress_batch(sub, **kw)
        assert np.isfinite(sm.energy).all() and (sm.sigma[:, 0] > 0).all()


# 1e15: the fp32 products (1e30 and their sums) stay finite.  1e20 at N = 20: they overflow, the fp32-product Gram is
# not finite and the fp64 refinement pass decides -- the deltas are finite, the reference accepts them.
@pytest.mark.parametrize("N,scale", [(8, 1e15), (20, 1e15), (20, 1e20)])
def test_large_finite_deltas_do_not_raise(sq, orc, N, scale):
    D = 4101
    deltas = [(d * 100.0 * scale).cuda() for d in orc.synthetic_deltas(D, N, 500 + N)]
    assert all(bool(torch.isfinite(d).all()) for d in deltas) and float(deltas[0].abs().max()) > 0.01 * scale
    plan, sm = sq.compress_batch([deltas], energy_threshold=0.9, max_rank=None, center=True, fp16=True, low_bits=4,
                                 rtvq_stages=2, device="cuda")
    assert np.isfinite(sm.energy[0]) and 0.0 < sm.energy[0] <= 1.0
    r = int(sm.r[0])
    assert 1 <= int(sm.k[0]) <= r == N
    S_ref = _s64(deltas, True)
    real = S_ref > 1e-5 * S_ref[0]
    real[-1] = False                 # the null direction centring creates: numerical noise in LAPACK, 0 here
    print(f"N={N} scale={scale:g}: max rel sigma error "
          f"{np.max(np.abs(sm.sigma[0, :r][real] - S_ref[real]) / S_ref[real]):.3e}, energy {sm.energy[0]:.6f}")
    np.testing.assert_allclose(sm.sigma[0, :r][real], S_ref[real], rtol=2e-5)      # test_hip_parity.py's sigma rtol
    # and through the dictionary API
    tv = {f"task{t:02d}": {"w": d} for t, d in enumerate(deltas)}
    bases, _ = sq.driver.run_basis_and_compress(tv, None, _cfg(sq), "cuda")
    assert np.isfinite(bases["w"]["masked"]["energy_retained"])


# ------------------------------------------------------------------------------------------- staged ABI
@pytest.mark.parametrize("N", [8, 20])
def test_staged_range_entry_points_through_ctypes(sq, N):
    """svdq_gram_center_range + svdq_eig_rank_select_range over two halves of a plan: the flag is written by every
    eigen stage, so it is exact per parameter and a clean rerun on the same workspace and small buffer clears it."""
    vectors = _ragged(N, 200 + N)
    plan = sq.pipeline.CompressPlan(ROWS, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4,
                                    rtvq_stages=2, device="cuda")
    table = plan.pointer_table(vectors)
    st = torch.cuda.current_stream()
    P, half = len(ROWS), 2

    def staged():
        for p0, n in ((0, half), (half, P - half)):
            plan.gram_range(table, p0, n, st)
            plan.eig_range(table, p0, n, st)
        return _host_small(sq, plan)["energy"].copy()

    for p in (1, 3):                                     # one in each half
        keep = vectors[p][0][ROWS[p] - 1].clone()
        vectors[p][0][ROWS[p] - 1] = float("nan")
        en = staged()
        assert np.isnan(en).tolist() == [q == p for q in range(P)], (p, en)
        assert sq.pipeline.nonfinite_parameters(plan.small, plan.layout, P) == [p]
        vectors[p][0][ROWS[p] - 1] = keep
        en = staged()
        assert np.isfinite(en).all(), en


# ------------------------------------------------------------------------------------------- the reference's callables
def test_basis_callables_raise(sq):
    g = torch.Generator(device="cuda").manual_seed(3)
    deltas = [0.01 * torch.randn(4101, generator=g, device="cuda") for _ in range(8)]
    deltas[5][4100] = float("nan")
    with pytest.raises(RuntimeError, match=WORDING):
        sq.construct_basis(deltas, energy_threshold=0.9, max_rank=None, center=True, device="cuda", verbose=False)
    with pytest.raises(RuntimeError, match=WORDING):
        sq.construct_basis([d.cpu() for d in deltas], device="cpu", verbose=False)
    clean = [d.nan_to_num() for d in deltas]
    with pytest.raises(RuntimeError, match=WORDING):
        sq.construct_masked_basis(deltas, None, device="cuda")
    with pytest.raises(RuntimeError, match=WORDING):                      # the noise region alone holds it
        sq.construct_masked_basis(clean, deltas, device="cuda", include_noise=True)
    assert sq.construct_masked_basis(clean, deltas, device="cuda", include_noise=False)["noise"] is None
    M = torch.stack(deltas, dim=1)                                        # [D, N]
    with pytest.raises(RuntimeError, match=WORDING):
        sq.compute_svd(M)
    U, S, Vh = sq.compute_svd(torch.stack(clean, dim=1))
    assert torch.isfinite(S).all() and U.shape == (4101, 8)


def test_cli_raises_on_a_checkpoint_with_nan(sq, tmp_path, orc):
    tasks = ["Cars", "DTD", "EuroSAT", "GTSRB"]
    g = torch.Generator().manual_seed(5)
    shapes = {"blk.attn.weight": (96, 64), "blk.attn.bias": (96,), "ln.weight": (64,)}
    base = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    ck = tmp_path / "ckpt"
    ck.mkdir()
    torch.save(base, tmp_path / "base.pt")
    deltas = {k: orc.synthetic_deltas(int(np.prod(s)), len(tasks), 800 + i) for i, (k, s) in enumerate(shapes.items())}
    for ti, t in enumerate(tasks):
        sd = {k: base[k] + deltas[k][ti].view(shapes[k]) for k in shapes}
        if t == "EuroSAT":
            sd["blk.attn.bias"][40] = float("nan")
        torch.save(sd, ck / f"{t}.pt")
    argv = ["--tasks", *tasks, "--checkpoint-dir", str(ck), "--base-model-path", str(tmp_path / "base.pt"),
            "--energy-threshold", "0.9", "--max-rank", "2", "--low-bits", "4", "--rtvq-stages", "2",
            "--output-dir", str(tmp_path / "out"), "--artifact-dir", str(tmp_path / "art")]
    with pytest.raises(RuntimeError, match=WORDING) as ei:
        sq.cli.main(argv)
    msg = str(ei.value)
    assert "'blk.attn.bias'" in msg and "blk.attn.weight" not in msg and "ln.weight" not in msg, msg
    assert not (tmp_path / "out" / "merged_state_dict.pt").exists()
