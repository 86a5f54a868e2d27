"""
The ``svd_min_mask_size`` gate of ``driver.build_bases`` against the reference's own run
(tests/golden/pipeline_gates.npz, written by make_golden_gates.py): union masks with exactly 0, 9 and 10 set elements
at svd_min_mask_size = 10, a mask with every element set (empty noise region), an ordinary dense mask and an unmasked
parameter, with and without the noise region.  The key sets of ``bases`` and ``compressed_all`` and the None pattern
must be the fixture's; the numbers are held to the bounds of test_hip_parity.py::test_pipeline_vs_reference_vectors.
"""
import json

import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu

MSE_TOL = 1e-6      # test_hip_parity.py's bound on the reconstruction MSE against the reference's


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


@pytest.mark.parametrize("case", ["noise1", "noise0"])
def test_gate_vs_reference_vectors(sq, case):
    g = load_golden("pipeline_gates.npz")
    assert f"{case}__raised" not in g
    tasks = [str(t) for t in g["tasks"]]
    params = [str(p) for p in g["params"]]
    layout = json.loads(str(g[f"{case}__layout_json"]))
    cfg = sq.SVDHybridConfig(svd_energy_threshold=0.9, svd_max_rank=64, svd_center=True, svd_fp16=True,
                             svd_low_bits=4, svd_rtvq_stages=2, svd_include_noise=(case == "noise1"),
                             svd_min_mask_size=int(g["min_mask_size"]))
    task_vectors = {t: {} for t in tasks}
    masks = {}
    for pname in params:
        x = g[f"in__{pname}"]
        shape = g[f"mask__{pname}"].shape if f"mask__{pname}" in g else (x.shape[1],)
        for i, t in enumerate(tasks):
            task_vectors[t][pname] = torch.from_numpy(x[i]).view(*shape).cuda()
        if f"mask__{pname}" in g:
            masks[pname] = torch.from_numpy(g[f"mask__{pname}"]).cuda()
    bases, comp = sq.run_basis_and_compress(task_vectors, masks, cfg, "cuda")
    assert sorted(bases.keys()) == layout["bases"]
    assert sorted(comp.keys()) == layout["compressed"]
    quant = sq.RTVQQuantizer(4, 2)
    n_ok = n_all = 0
    for pname in layout["compressed"]:
        lay = layout["params"][pname]
        for region in ("masked", "noise"):
            want_keys = lay[f"basis_{region}"]
            b = bases[pname][region]
            if want_keys is None:
                assert b is None, (pname, region)
                continue
            assert b is not None and set(want_keys) <= set(b.keys()), (pname, region)
            tag = f"{case}__basis__{pname}__{region}__"
            assert b["k"] == int(g[tag + "k"]), (pname, region)
            assert b["D"] == int(g[tag + "D"]), (pname, region)
            assert abs(b["energy_retained"] - float(g[tag + "energy"])) < 2e-5, (pname, region)
            S_ref = g[tag + "S"]
            real = S_ref > 1e-5 * S_ref[0]
            np.testing.assert_allclose(b["singular_values"].cpu().numpy()[real], S_ref[real], rtol=2e-5)
            assert b["U_high"].dtype == torch.float16 and b["mean"].shape == (b["D"], 1)
        assert list(comp[pname].keys()) == tasks
        for t in tasks:
            art, want = comp[pname][t], lay[t]
            assert sorted(art.keys()) == sorted(want.keys())
            for region, bkey in (("masked", "masked"), ("unmasked", "noise")):
                if want[region] is None:
                    assert art[region] is None, (pname, t, region)
                    continue
                assert art[region] is not None and sorted(art[region].keys()) == want[region], (pname, t, region)
                a, b = art[region], bases[pname][bkey]
                tag = f"{case}__coef__{pname}__{t}__{region}__"
                assert a["c_high_fp16"].dtype == torch.float16 and a["c_high_fp16"].shape == g[tag + "c_high_fp16"].shape
                q = a["c_low_quant"]
                assert q["num_bits"] == 4 and q["num_stages"] == 2 and len(q["payloads"]) == int(g[tag + "n_payloads"])
                rec = sq.reconstruct_from_coefficients(a["c_high_fp16"].cuda().float(),
                                                       quant.dequantize(q, device="cuda").float(), b["U_high"],
                                                       b["U_low"], "cuda", mean=b["mean"]).cpu().numpy()
                ref = g[tag + "recon"]
                # the rule of test_hip_parity.py::_compare_recon: MSE where both are finite; with n_low <= 2 the
                # degenerate quantizer may go NaN on either side
                of, rf = np.isfinite(rec).all(), np.isfinite(ref).all()
                if of and rf:
                    mse = float(np.mean((rec - ref) ** 2))
                    assert mse <= MSE_TOL, (pname, t, region, mse)
                    n_ok += 1
                else:
                    assert b["U_low"].shape[1] <= 2 or (of == rf), (pname, t, region, of, rf)
                n_all += 1
    assert n_ok >= 0.75 * n_all, (n_ok, n_all)
