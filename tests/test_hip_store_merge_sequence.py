"""
The four merges over every task's own values back to back on ONE adopted store: TIES, DARE, the consensus merge with its
TALL masks, and EMR share the coefficient kernel (k_store_coeff), the plan's coefficient work buffer and the host
front-end, so a call must leave nothing behind that the next one reads.  Every tensor, mask stream and statistic of a call
inside the sequence -- in the order above, then in reverse on the same adoption -- equals, bit for bit, what the same
call returns on a fresh adoption of the same store.

Shapes: rows 1, 65 (one ballot + 1), 129 (the 128-row block of 17+ tasks + 1), 513 (two 256-row blocks + 1), so every
later parameter starts at a bit offset that is no multiple of 32; one task lacks one parameter, so adoption makes two
plans and the slot tables have an empty slot; fp16 basis; 3 tasks (one group of 4, 4 rows per lane) and 17 tasks (three
groups of 8, 2 rows per lane in the plan of 17 and 4 in the plan of 16).  The stores are built as
tests/test_hip_tall_consensus.py builds them (k capped at 1, one residual stage), and what they merge to is asserted
finite.  That decides which parameter a task lacks: the quantizer writes non-finite values where the low part is one
coefficient (tests/test_hip_ties_merge.py), which is what a parameter of two tasks has at k = 1 unless it has a single
row (r = 1, no low part) -- so at 3 tasks it is the one-row parameter, at 17 tasks the one of 129 rows.
"""
import math

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


def _calls(sq, T, base):
    lam = min(0.4, 1.0 / math.sqrt(T - 1))
    return {
        "ties": lambda b, c, cfg: sq.ties_merge_parameters(c, b, SHAPES, cfg, density=0.3, base_state_dict=base,
                                                           device="cuda", return_stats=True),
        "dare": lambda b, c, cfg: sq.dare_merge_parameters(c, b, SHAPES, cfg, drop_rate=0.5, seed=11, scaling=0.7,
                                                           base_state_dict=base, device="cuda", return_stats=True),
        "consensus": lambda b, c, cfg: sq.consensus_merge_parameters(c, b, SHAPES, cfg, tall_lambda=lam, k=2,
                                                                     base_state_dict=base, return_masks=True,
                                                                     device="cuda", return_stats=True),
        "emr": lambda b, c, cfg: sq.emr_merge_parameters(c, b, SHAPES, cfg, device="cuda", return_stats=True),
    }


def _assert_same(got, want, where):
    """Tensors bit for bit (NaN payloads included), everything else equal, through tuples and dictionaries."""
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
        assert type(got) is type(want) and got == want, where      # statistics: ints and floats, exactly


@pytest.mark.parametrize("T", [3, 17])
def test_back_to_back_merges_equal_fresh_adoptions(sq, tmp_path, T):
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
    calls = _calls(sq, T, base)
    # ---- every call alone, each on an adoption of its own
    fresh = {}
    for name, call in calls.items():
        b, c, acfg = _adopt(sq, d)
        plans = {id(c[n]._batch[0].plan) for n in NAMES}
        assert len(plans) == 2, "the parameter one task lacks sits in a plan of its own"
        fresh[name] = call(b, c, acfg)
        for x in fresh[name][0].values():      # the merged / elected tensors
            assert x.is_cuda and bool(torch.isfinite(x).all()), name
    assert fresh["consensus"][2]["rows"] == fresh["emr"][3]["rows"] == sum(ROWS)
    assert any(bool(m.any()) for m in fresh["consensus"][1].values())      # the streams are not empty
    assert any(bool(m.any()) for m in fresh["emr"][1].values())
    # ---- the sequence on one adoption, forwards and backwards
    b, c, acfg = _adopt(sq, d)
    order = list(calls)
    for name in order + order[::-1]:
        _assert_same(calls[name](b, c, acfg), fresh[name], (T, name))
