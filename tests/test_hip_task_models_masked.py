"""
GPU tests of the dictionary level of masked task reconstruction: merge.reconstruct_task_vectors_masked (fused_masks=True),
storage.reconstruct_tasks_from_artifacts_masked and scripts/reconstruct_tasks.py --mask-dir.  A
masked parameter of a fused run, or of stored artifacts adopted with the caller's masks, gets reconstruct_from_masked and
``base +`` inside ONE svdq_task_reconstruct_masked per plan.  The truth in every case is the per-parameter route on that
task alone (tests/test_hip_task_models.py),

    base + merge_parameter(name, {t: comp[name][t]}, bases[name], {t: 1.0}, quantizer, shape, mask=..., ...)

and the comparison is bit for bit.  Sizes 4097 and 70001 with masks of density 0.6; 8 tasks (the signal regions are
walked, the noise regions went through index lists: two plans) and 17 (index lists for both: one plan holds both
regions); with and without noise regions.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"m04097": 4097, "m70001": 70001}
SETUPS = [(8, True), (8, False), (17, True), (17, False)]
NAMES = ("svdq_task_reconstruct_masked", "svdq_task_reconstruct", "svdq_reconstruct", "svdq_rtvq_dequantize", "svdq_merge")


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


def _tasks(n):
    return [f"t{i:02d}" for i in range(n)]


class _Spy:
    """Counters on the library's own entry points and on mask_loader.reconstruct_from_masked."""

    def __init__(self, sq):
        self.lib, self.ml = sq._native.lib(), sq.mask_loader
        self.calls = dict.fromkeys(NAMES + ("reconstruct_from_masked",), 0)

    def __enter__(self):
        self.real = {n: getattr(self.lib, n) for n in NAMES}
        for n in NAMES:
            setattr(self.lib, n, self._wrap(n, self.real[n]))
        self.scatter = self.ml.reconstruct_from_masked
        self.ml.reconstruct_from_masked = self._wrap("reconstruct_from_masked", self.scatter)
        return self.calls

    def _wrap(self, n, real):
        def call(*a, **kw):
            self.calls[n] += 1
            return real(*a, **kw)
        return call

    def __exit__(self, *exc):
        for n in NAMES:
            setattr(self.lib, n, self.real[n])
        self.ml.reconstruct_from_masked = self.scatter


def _counts(**some):
    return dict(dict.fromkeys(NAMES + ("reconstruct_from_masked",), 0), **some)


_RUNS = {}


def _run(sq, n, noise, tmp_path_factory):
    """One fused run per setup, its artifacts written once, and the truth of every (parameter, task) by the
    per-parameter route from the artifacts as LOADED; shared by the tests and left unchanged."""
    if (n, noise) in _RUNS:
        return _RUNS[(n, noise)]
    from oracle import svd_hybrid_oracle as orc
    tasks = _tasks(n)
    g = torch.Generator().manual_seed(6)
    tv = {t: {} for t in tasks}
    masks = {}
    for name, rows in SIZES.items():
        for t, x in zip(tasks, orc.synthetic_deltas(rows, n, 77 + rows)):
            tv[t][name] = x.cuda()
        masks[name] = (torch.rand(rows, generator=g) < 0.6).cuda()
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=None, svd_low_bits=4, svd_rtvq_stages=2,
                             svd_include_noise=noise, svd_noise_shrink=0.5, svd_min_mask_size=10)
    bases, comp = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    shapes = {name: torch.Size([r]) for name, r in SIZES.items()}
    base = {name: torch.randn(r, generator=g).cuda() for name, r in SIZES.items()}
    d = str(tmp_path_factory.mktemp(f"n{n}{'noise' if noise else ''}") / "art")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {k: {"original_shape": list(s)} for k, s in shapes.items()}}, cfg, d)
    art = sq.load_all_artifacts(d, device="cpu")
    q = sq.RTVQQuantizer(num_bits=cfg.svd_low_bits, num_stages=cfg.svd_rtvq_stages)
    truth = {name: {t: base[name] + sq.merge_parameter(name, {t: art["compressed"][name][t]}, art["bases"][name], {t: 1.0}, q,
                                                       shapes[name], mask=masks[name], include_noise=noise,
                                                       noise_shrink=cfg.svd_noise_shrink, device="cuda")
                    for t in tasks} for name in SIZES}
    if noise:      # the noise region matters: the rows outside the mask are not the base's
        outside = (truth["m70001"][tasks[0]] - base["m70001"])[~masks["m70001"]]
        assert float(outside.abs().max()) > 0
    _RUNS[(n, noise)] = (cfg, bases, comp, masks, shapes, d, tasks, base, truth)
    return _RUNS[(n, noise)]


def _plans(bases, noise):
    return {id(bases[name][r]._batch[0].plan) for name in SIZES for r in (("masked", "noise") if noise else ("masked",))}


def _assert_equal(got, truth, tasks):
    assert list(got) == list(tasks)
    for t in tasks:
        assert sorted(got[t]) == sorted(truth)
        for name in truth:
            v = got[t][name]
            assert v.is_cuda and v.shape == truth[name][t].shape and _bits(v, truth[name][t]), (t, name)


@pytest.mark.parametrize("n,noise", SETUPS)
def test_fused_run_with_the_masks_it_compressed_with(sq, n, noise, tmp_path_factory):
    cfg, bases, comp, masks, shapes, d, tasks, base, truth = _run(sq, n, noise, tmp_path_factory)
    plans = len(_plans(bases, noise))
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(comp, bases, masks, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls == _counts(svdq_task_reconstruct_masked=plans), calls
    _assert_equal(got, truth, tasks)
    # the outputs are the call's own: a second call (a subset, no base) leaves them alone
    held = {t: {k: v.clone() for k, v in got[t].items()} for t in tasks}
    pick = [tasks[-1], tasks[0]]
    again = sq.reconstruct_task_vectors_masked(comp, bases, masks, shapes, cfg, tasks=pick, device="cuda")
    torch.cuda.synchronize()
    assert list(again) == pick
    for t in pick:
        for name in SIZES:
            assert _bits(base[name] + again[t][name], truth[name][t]), (t, name)
    for t in tasks:
        for name in SIZES:
            assert _bits(got[t][name], held[t][name]), (t, name)
    # the default keyword keeps the compacted route: one svdq_task_reconstruct per plan, one scatter per (parameter, task)
    with _Spy(sq) as calls:
        plain = sq.reconstruct_task_vectors(comp, bases, masks, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls == _counts(svdq_task_reconstruct=plans, reconstruct_from_masked=len(SIZES) * n), calls
    _assert_equal(plain, truth, tasks)


@pytest.mark.parametrize("n,noise", [(8, True), (17, False)])
def test_another_mask_object_takes_the_compacted_route(sq, n, noise, tmp_path_factory):
    cfg, bases, comp, masks, shapes, d, tasks, base, truth = _run(sq, n, noise, tmp_path_factory)
    clones = {name: m.clone() for name, m in masks.items()}
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(comp, bases, clones, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls == _counts(svdq_task_reconstruct=len(_plans(bases, noise)), reconstruct_from_masked=len(SIZES) * n), calls
    _assert_equal(got, truth, tasks)
    # one parameter with the run's own mask, one with a clone: each takes its route
    mixed = {"m04097": masks["m04097"], "m70001": clones["m70001"]}
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(comp, bases, mixed, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls["svdq_task_reconstruct_masked"] >= 1 and calls["reconstruct_from_masked"] == n, calls
    _assert_equal(got, truth, tasks)


@pytest.mark.parametrize("n,noise", SETUPS)
def test_stored_artifacts_adopted_with_the_callers_masks(sq, n, noise, tmp_path_factory):
    cfg, _, _, masks, shapes, d, tasks, base, truth = _run(sq, n, noise, tmp_path_factory)
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda", masks=masks)
    plans = len(_plans(ab, noise))
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(ac, ab, masks, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls == _counts(svdq_task_reconstruct_masked=plans), calls
    _assert_equal(got, truth, tasks)
    # equal masks in other tensors fit as well: what counts for stored artifacts is the stored row count
    clones = {name: m.clone() for name, m in masks.items()}
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(ac, ab, clones, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls == _counts(svdq_task_reconstruct_masked=plans), calls
    _assert_equal(got, truth, tasks)
    # plans adopted WITHOUT the masks hold compacted rows only: the compacted route, the same bits
    pb, pc = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda")
    with _Spy(sq) as calls:
        got = sq.reconstruct_task_vectors_masked(pc, pb, masks, shapes, cfg, device="cuda", base_state_dict=base)
    assert calls["svdq_task_reconstruct_masked"] == 0 and calls["svdq_task_reconstruct"] == len(_plans(pb, noise)), calls
    _assert_equal(got, truth, tasks)
    # and the reload entry point hands masks and keyword through
    with _Spy(sq) as calls:
        models = sq.reconstruct_tasks_from_artifacts_masked(d, base, masks, tasks=[tasks[2]], device="cuda")
    assert calls == _counts(svdq_task_reconstruct_masked=plans), calls
    for name in SIZES:
        assert _bits(models[tasks[2]][name], truth[name][tasks[2]]), name


def test_batched_masked_merge_of_a_plan_that_holds_both_regions(sq, tmp_path_factory):
    """N = 17 with noise regions: index lists for both regions, so ONE plan holds the signal and the noise entry of both
    parameters and a plan entry's index is not its mask's index.  The unit starts must be looked up by mask
    (driver.build_bases): the batched masked merge equals the per-parameter route on every parameter, not the first only."""
    cfg, bases, comp, masks, shapes, d, tasks, base, truth = _run(sq, 17, True, tmp_path_factory)
    assert len(_plans(bases, True)) == 1
    w = {t: 1.0 / len(tasks) for t in tasks}
    with _Spy(sq) as calls:
        fast = sq.merge_all_parameters(comp, bases, masks, w, shapes, cfg, device="cuda", verbose=False)
    assert calls["reconstruct_from_masked"] == 0, calls      # the scatter happened inside svdq_merge_masked
    plain = {name: {t: dict(a) for t, a in v.items()} for name, v in comp.items()}
    slow = sq.merge_all_parameters(plain, bases, masks, w, shapes, cfg, device="cuda", verbose=False)
    for name in SIZES:
        assert _bits(fast[name], slow[name]), name


def _outcome(fn):
    """("raised", exception type) or ("returned", result) of a call, the device drained either way."""
    try:
        res = fn()
        torch.cuda.synchronize()
        return "returned", res
    except Exception as exc:      # whatever the compacted route raises is the contract here
        return "raised", type(exc)


@pytest.mark.parametrize("n,noise", [(8, True), (17, False)])
def test_a_mask_that_does_not_fit_the_stored_rows_keeps_the_compacted_route(sq, n, noise, tmp_path_factory):
    """A mask with one more set element than the stored signal rows: the parameter is not walked -- it keeps the compacted
    route and so does whatever that route does on this input (the same exception type if it raises, the same bits if
    it returns: svdq_mask_expand reads the one spare element its caller appends, so today it returns)."""
    cfg, _, _, masks, shapes, d, tasks, base, truth = _run(sq, n, noise, tmp_path_factory)
    wrong = {name: m.clone() for name, m in masks.items()}
    first_clear = int((~wrong["m70001"]).nonzero()[0])
    wrong["m70001"][first_clear] = True
    art = sq.load_all_artifacts(d, device="cpu")
    ab, ac = sq.adopt_artifacts(art["bases"], art["compressed"], cfg, device="cuda", masks=wrong)
    kinds = []
    for fused in (False, True):
        with _Spy(sq) as calls:
            kinds.append(_outcome(lambda: sq.reconstruct_task_vectors_masked(ac, ab, wrong, shapes, cfg, device="cuda",
                                                                      base_state_dict=base, fused_masks=fused)))
        if fused:      # the parameter whose mask fits is walked, the other one is not
            assert calls["svdq_task_reconstruct_masked"] >= 1, calls
            assert calls["reconstruct_from_masked"] == (n if kinds[-1][0] == "returned" else 1), calls
    assert kinds[0][0] == kinds[1][0], kinds
    if kinds[0][0] == "raised":
        assert kinds[0][1] is kinds[1][1], kinds
    else:
        for t in tasks:
            assert _bits(kinds[1][1][t]["m70001"], kinds[0][1][t]["m70001"]), t
            assert _bits(kinds[1][1][t]["m04097"], truth["m04097"][t]), t


def test_script_writes_every_task_model_of_a_masked_run(sq, tmp_path, tmp_path_factory):
    """scripts/reconstruct_tasks.py --mask-dir as a user would call it: per-task mask files whose union is the combined
    mask of the run, a base checkpoint with one key the artifacts do not cover."""
    cfg, _, _, masks, shapes, d, tasks, base, truth = _run(sq, 8, True, tmp_path_factory)
    mask_dir = tmp_path / "masks"
    mask_dir.mkdir()
    g = torch.Generator().manual_seed(11)
    for i, t in enumerate(tasks):      # every task drops a random tenth of the union; the first keeps it whole
        pm = {name: (m.cpu() & (torch.rand(m.numel(), generator=g) > (0.1 if i else -1.0))) for name, m in masks.items()}
        torch.save(pm, str(mask_dir / f"{t}_mask.pt"))
    cpu_base = {name: b.cpu() for name, b in base.items()}
    cpu_base["head.bias"] = torch.randn(10, generator=g)
    torch.save(cpu_base, str(tmp_path / "base.pt"))
    out = str(tmp_path / "models")
    rc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reconstruct_tasks.py"), "--artifact-dir", d,
                         "--base-model-path", str(tmp_path / "base.pt"), "--output-dir", out, "--device", "cuda",
                         "--mask-dir", str(mask_dir), "--mask-strategy", "union"],
                        capture_output=True, text=True, timeout=600)
    assert rc.returncode == 0, rc.stderr[-2000:]
    assert sorted(os.listdir(out)) == [f"{t}.pt" for t in tasks]
    for t in tasks:
        sd = torch.load(os.path.join(out, f"{t}.pt"), weights_only=True)
        assert sorted(sd) == sorted(cpu_base)
        for name in SIZES:
            assert _bits(sd[name].cuda(), truth[name][t]), (t, name)
        assert _bits(sd["head.bias"], cpu_base["head.bias"])
