"""
tests/golden/make_golden_gates.py -- regenerates tests/golden/pipeline_gates.npz by running the REFERENCE itself.

Run only where the reference checkout is mounted (make_golden.py says where and why its package needs the stub
modules below); the tests never import the reference, they read the fixture.  No reference source is stored.

pipeline_gates.npz pins the ``svd_min_mask_size`` gate of Step 4 + Step 5 (cli.py:317-363 with the guard of
cli.py:343, compress.py:130-170, basis.py:438-468) on a toy model of 4 tasks whose union masks have exactly 0, 9
and 10 set elements, one mask with every element set (an empty noise region), one ordinary dense mask and one
unmasked parameter; svd_min_mask_size = 10, run once with svd_include_noise True ("noise1") and once False
("noise0").  Per case: which parameters exist in ``bases`` / ``compressed_all`` and which regions are None
(``<case>__layout_json``), and the numbers the way pipeline.npz records them.  A case the reference itself raises on
is recorded as ``<case>__raised`` = the exception's type name instead of numbers.
"""
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

sys.dont_write_bytecode = True
sys.path.insert(0, REF)
for _name, _path in (("src", REF + "/src"), ("src.svd_hybrid", REF + "/src/svd_hybrid")):
    _m = types.ModuleType(_name)
    _m.__path__ = [_path]
    sys.modules[_name] = _m

from src.svd_hybrid import rtvq as ref_rtvq                      # noqa: E402
from src.svd_hybrid import basis as ref_basis                    # noqa: E402
from src.svd_hybrid import compress as ref_compress              # noqa: E402
from src.svd_hybrid import merge as ref_merge                    # noqa: E402
from src.svd_hybrid import mask_loader as ref_masks              # noqa: E402

sys.path.insert(0, ROOT)
from oracle.svd_hybrid_oracle import synthetic_deltas            # noqa: E402  (input generator only)

torch.set_num_threads(8)

TASKS = ["Cars", "DTD", "EuroSAT", "GTSRB"]
MIN_MASK_SIZE = 10
# name -> (shape, set elements of the union mask: a count, "all", "dense", or None = no mask)
PARAMS = {
    "g0.empty.weight": ((6, 8), 0),
    "g1.nine.weight": ((6, 8), 9),
    "g2.ten.weight": ((6, 8), 10),
    "g3.full.weight": ((6, 8), "all"),
    "g4.dense.weight": ((12, 8), "dense"),
    "g5.plain.bias": ((24,), None),
}


def payload_arrays(prefix, qobj, out):
    """The payload count alone: what each payload holds is pinned by pipeline.npz, and every array costs the
    archive a header."""
    out[prefix + "n_payloads"] = np.int64(len(qobj["payloads"]))


def union_mask(shape, want, g):
    """A union mask (compute_union_mask of per-task masks) with the wanted number of set elements."""
    numel = int(np.prod(shape))
    if want == "all":
        per_task = [torch.ones(shape, dtype=torch.bool) for _ in TASKS]
    elif want == "dense":
        per_task = [torch.rand(shape, generator=g) > 0.6 for _ in TASKS]
    else:
        # the wanted positions dealt out over the tasks, so that only the union has them all
        pos = torch.randperm(numel, generator=g)[:want]
        per_task = []
        for i in range(len(TASKS)):
            m = torch.zeros(numel, dtype=torch.bool)
            m[pos[i::len(TASKS)]] = True
            per_task.append(m.view(shape))
    mask = ref_masks.compute_union_mask(per_task)
    if isinstance(want, int):
        assert int(mask.sum()) == want, (int(mask.sum()), want)
    return mask


def run_case(task_vectors, masks, cfg, out, case):
    """The reference's Step 4 body (cli.py:317-363, guard of :343 included) and compress_all_parameters."""
    bases = {}
    for pname in sorted(PARAMS):
        mask = masks.get(pname)
        md, ud = [], []
        for t in TASKS:
            delta = task_vectors[t][pname]
            if mask is not None and mask.shape == delta.shape:
                if mask.sum() >= cfg.svd_min_mask_size:
                    md.append(ref_masks.apply_mask_to_tensor(delta, mask))
                    if cfg.svd_include_noise:
                        ud.append(ref_masks.get_unmasked_portion(delta, mask))
            else:
                md.append(delta.flatten())
        if md and len(md[0]) > 0:                                   # cli.py:343
            basis = ref_basis.construct_masked_basis(md, ud if cfg.svd_include_noise else None,
                                                     energy_threshold=cfg.svd_energy_threshold,
                                                     max_rank=cfg.svd_max_rank, center=cfg.svd_center,
                                                     device="cpu", include_noise=cfg.svd_include_noise)
            if cfg.svd_fp16 and basis.get("masked") is not None:
                for region in ("masked", "noise"):
                    if basis.get(region) is not None:
                        basis[region]["U_high"] = basis[region]["U_high"].half()
                        basis[region]["U_low"] = basis[region]["U_low"].half()
            bases[pname] = basis
    compressed = ref_compress.compress_all_parameters(task_vectors, masks, bases, cfg, device="cpu")
    quant = ref_rtvq.RTVQQuantizer(cfg.svd_low_bits, cfg.svd_rtvq_stages)
    layout = {"bases": sorted(bases), "compressed": sorted(compressed), "params": {}}
    for pname in sorted(compressed):
        lay = layout["params"][pname] = {}
        for region in ("masked", "noise"):
            b = bases[pname].get(region)
            lay[f"basis_{region}"] = None if b is None else sorted(b.keys())
            if b is not None:
                out[f"{case}__basis__{pname}__{region}__S"] = b["singular_values"].numpy()
                out[f"{case}__basis__{pname}__{region}__k"] = np.int64(b["k"])
                out[f"{case}__basis__{pname}__{region}__D"] = np.int64(b["D"])
                out[f"{case}__basis__{pname}__{region}__energy"] = np.float64(b["energy_retained"])
        for t in TASKS:
            art = compressed[pname][t]
            lay[t] = {r: (None if art[r] is None else sorted(art[r].keys())) for r in sorted(art.keys())}
            for region, bkey in (("masked", "masked"), ("unmasked", "noise")):
                a = art[region]
                if a is None:
                    continue
                tag = f"{case}__coef__{pname}__{t}__{region}__"
                out[tag + "c_high_fp16"] = a["c_high_fp16"].numpy()
                payload_arrays(tag, a["c_low_quant"], out)
                b = bases[pname][bkey]
                rec = ref_merge.reconstruct_from_coefficients(
                    a["c_high_fp16"].float(), quant.dequantize(a["c_low_quant"]).float(),
                    b["U_high"], b["U_low"], "cpu", mean=b["mean"])
                out[tag + "recon"] = rec.numpy()
    out[f"{case}__layout_json"] = np.array(json.dumps(layout, sort_keys=True))


def main():
    g = torch.Generator().manual_seed(11)
    task_vectors = {t: {} for t in TASKS}
    masks, out = {}, {}
    for pi, (pname, (shp, want)) in enumerate(sorted(PARAMS.items())):
        numel = int(np.prod(shp))
        ds = synthetic_deltas(numel, len(TASKS), 300 + pi)
        for t, d in zip(TASKS, ds):
            task_vectors[t][pname] = d.view(shp)
        out[f"in__{pname}"] = torch.stack(ds).numpy()
        if want is not None:
            masks[pname] = union_mask(shp, want, g)
            out[f"mask__{pname}"] = masks[pname].numpy()
    for case, noise in (("noise1", True), ("noise0", False)):
        cfg = types.SimpleNamespace(svd_low_bits=4, svd_rtvq_stages=2, svd_include_noise=noise,
                                    svd_min_mask_size=MIN_MASK_SIZE, svd_energy_threshold=0.9, svd_max_rank=64,
                                    svd_center=True, svd_fp16=True)
        try:
            run_case(task_vectors, masks, cfg, out, case)
        except Exception as exc:      # the reference's own failure on this case is the datum
            for key in [k for k in out if k.startswith(case + "__")]:
                del out[key]
            out[f"{case}__raised"] = np.array(type(exc).__name__)
            print(f"{case}: the reference raised {type(exc).__name__}: {exc}")
    out["tasks"] = np.array(TASKS)
    out["params"] = np.array(sorted(PARAMS))
    out["min_mask_size"] = np.int64(MIN_MASK_SIZE)
    path = os.path.join(HERE, "pipeline_gates.npz")
    np.savez_compressed(path, **out)
    print(f"wrote pipeline_gates.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
