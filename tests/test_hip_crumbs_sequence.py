"""
The Model Breadcrumbs merge back to back with TIES on ONE adopted store: both go through the coefficient kernel
(k_store_coeff), the plan's coefficient work buffer and the host front-end of the merges over every task's own values,
so a call must leave nothing behind that the next one reads.  Breadcrumbs, then TIES, then Breadcrumbs (with other
arguments: the second call finds the work buffer as TIES left it): every tensor and statistic equals, bit for bit, what
the same call returns on a fresh adoption of the same store.

The stores are those of tests/test_hip_store_merge_sequence.py: rows 1, 65, 129, 513, one task lacks one parameter (two
plans, an empty slot in the slot tables), fp16 basis, k capped at 1 and one residual stage; 3 tasks (one group of 4) and
17 tasks (three groups of 8: one bound per histogram launch in the plan of 17, both in the plan of 16).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 65, 129, 513]
NAMES = [f"p{rows:05d}" for rows in ROWS]
SHAPES = {n: torch.Size([r]) for n, r in zip(NAMES, ROWS)}
LACKING = {3: "p00001", 17: "p00129"}


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _adopt(sq, d):
    art = sq.load_all_artifacts(d, device="cuda")
    bases, comp = sq.adopt_artifacts(art["bases"], art["compressed"], art["config"], device="cuda")
    return bases, comp, art["config"]


def _calls(sq, base):
    return {
        "crumbs": lambda b, c, cfg: sq.breadcrumbs_merge_parameters(c, b, SHAPES, cfg, density=0.8, gamma=0.05,
                                                                    base_state_dict=base, device="cuda",
                                                                    return_stats=True),
        "ties": lambda b, c, cfg: sq.ties_merge_parameters(c, b, SHAPES, cfg, density=0.3, base_state_dict=base,
                                                           device="cuda", return_stats=True),
        "crumbs_elected": lambda b, c, cfg: sq.breadcrumbs_merge_parameters(c, b, SHAPES, cfg, density=0.3, gamma=0.0,
                                                                            scaling=0.7, sign_election=True,
                                                                            merge_func="mean", device="cuda",
                                                                            return_stats=True),
    }


def _assert_same(got, want, where):
    """Tensors bit for bit, everything else equal, through tuples and dictionaries."""
    if isinstance(want, torch.Tensor):
        assert isinstance(got, torch.Tensor) and got.dtype is want.dtype and got.shape == want.shape, where
        a, b = got.cpu().contiguous().reshape(-1), want.cpu().contiguous().reshape(-1)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), where
    elif isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), where
        for key in want:
            _assert_same(got[key], want[key], where + (key,))
    elif isinstance(want, (tuple, list)):
        assert type(got) is type(want) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, where + (i,))
    else:
        assert type(got) is type(want) and got == want, where      # statistics: ints, floats and None, exactly


@pytest.mark.parametrize("T", [3, 17])
def test_breadcrumbs_ties_breadcrumbs_equal_fresh_adoptions(sq, tmp_path, T):
    from oracle import svd_hybrid_oracle as orc
    tasks = [f"t{i:02d}" for i in range(T)]
    tv = {t: {} for t in tasks}
    for rows in ROWS:
        for t, d in zip(tasks, orc.synthetic_deltas(rows, T, 53 * T + rows, rank=3)):
            tv[t][f"p{rows:05d}"] = d.cuda()
    del tv[tasks[1]][LACKING[T]]
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_low_bits=4, svd_fp16=True, svd_max_rank=1,
                             svd_rtvq_stages=1)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    d = str(tmp_path / "store")
    sq.save_all_artifacts(bases, comp, {"per_parameter": {n: {"original_shape": list(s)} for n, s in SHAPES.items()}},
                          cfg, d)
    del bases, comp
    g = torch.Generator().manual_seed(5 + T)
    base = {n: torch.randn(s, generator=g).cuda() for n, s in SHAPES.items()}
    calls = _calls(sq, base)
    # ---- every call alone, each on an adoption of its own
    fresh = {}
    for name, call in calls.items():
        b, c, acfg = _adopt(sq, d)
        plans = {id(c[n]._batch[0].plan) for n in NAMES}
        assert len(plans) == 2, "the parameter one task lacks sits in a plan of its own"
        fresh[name] = call(b, c, acfg)
        for x in fresh[name][0].values():
            assert x.is_cuda and bool(torch.isfinite(x).all()), name
    assert fresh["crumbs"][1]["rows"] == fresh["ties"][1]["rows"] == sum(ROWS)
    assert 0 < sum(fresh["crumbs"][1]["kept_total"].values()) < T * sum(ROWS)      # the band does something
    # ---- the sequence on one adoption, then once more
    b, c, acfg = _adopt(sq, d)
    for name in list(calls) * 2:
        _assert_same(calls[name](b, c, acfg), fresh[name], (T, name))
