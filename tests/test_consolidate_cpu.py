"""CPU tests of the host logic behind svdq_plan_consolidate_eig / svdq_plan_rebase: the agreement of include/svdq.h with
the ctypes binding (signatures and the layout struct), the flags of scripts/consolidate.py, the pure dictionary functions
(``compress.consolidate_task_list``, ``keep_row``, ``pipeline.keep_table``, ``consolidate_views``,
``storage.consolidated_config`` / ``consolidated_diagnostics``), every ``ValueError`` that comes before anything runs,
and the in-place write going through a temporary directory."""

import ctypes
import inspect
import os
import re
import sys
from ctypes import c_float, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _basis(D, k, n_low, N=None):
    return {"U_high": torch.zeros(D, k, dtype=torch.float16), "U_low": torch.zeros(D, n_low, dtype=torch.float16),
            "singular_values": torch.ones(k + n_low), "k": k, "mean": torch.zeros(D, 1), "energy_retained": 0.9, "D": D,
            "N": (k + n_low) if N is None else N}


def test_header_binding_and_layout_struct_agree():
    import svdq_amd
    nat = svdq_amd._native
    text = open(os.path.join(ROOT, "include", "svdq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ctype_of = {"int32_t": c_int32, "float": c_float}
    for name in ("svdq_plan_consolidate_layout", "svdq_plan_consolidate_eig", "svdq_plan_rebase"):
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert m.group(1) == "int"
        params = [a.strip() for a in m.group(2).split(",")]
        res, args = nat.SIGNATURES[name]
        assert res is c_int32
        assert len(args) == len(params), (name, params)
        for a, prm in zip(args, params):
            if "*" in prm:
                assert a is c_void_p or issubclass(a, ctypes._Pointer), (name, prm)
            else:
                assert a is ctype_of[prm.split()[0]], (name, prm)
    m = re.search(r"typedef struct svdq_consolidate_layout \{(.*?)\} svdq_consolidate_layout;", code, flags=re.S)
    fields = re.findall(r"int64_t\s+(\w+)\s*;", m.group(1))
    assert fields == [f for f, _ in nat.SvdqConsolidateLayout._fields_]
    assert all(t is c_int64 for _, t in nat.SvdqConsolidateLayout._fields_)
    assert "#define SVDQ_ABI_VERSION 1" in code
    lib = nat.lib()
    for name in ("svdq_plan_consolidate_layout", "svdq_plan_consolidate_eig", "svdq_plan_rebase"):
        assert hasattr(lib, name)
    for meth in ("consolidate", "consolidate_eig", "rebase", "consolidate_layout"):
        assert hasattr(svdq_amd.CompressPlan, meth)
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(svdq_amd.CompressPlan.consolidate) == [("self", E), ("dst_plan", E), ("keep", E), ("min_sigma", 0.0),
                                                      ("rows_dev", None)]
    assert sig(svdq_amd.consolidate_bases) == [("compressed_all", E), ("bases", E), ("config", E), ("tasks", None),
                                               ("min_sigma", 0.0), ("device", "cuda")]
    assert sig(svdq_amd.consolidate_artifacts)[:9] == [
        ("artifact_dir", E), ("output_dir", None), ("tasks", None), ("energy_threshold", None), ("max_rank", None),
        ("low_bits", None), ("rtvq_stages", None), ("center", None), ("min_sigma", 0.0)]


def test_rebase_table_views_follow_the_layout():
    from svdq_amd.pipeline import consolidate_views
    from svdq_amd import _native as nat
    P = 3
    lay, off = nat.SvdqConsolidateLayout(), 0
    sizes = {"w_off": P * 33 * 32 * 4, "bbar_off": P * 33 * 4, "r_off": P * 4, "k_off": P * 4, "live_off": P * 4,
             "dropped_off": P * 8, "eta_off": P * 8, "lambda_off": P * 32 * 8}
    for f, n in sizes.items():
        setattr(lay, f, off)
        off = (off + n + 255) // 256 * 256
    lay.total_bytes = off
    host = np.zeros(off, dtype=np.uint8)
    v = consolidate_views(host, lay, P)
    assert v.w.shape == (P, 33, 32) and v.bbar.shape == (P, 33) and v.lam.shape == (P, 32)
    v.r[2], v.k[2], v.live[1] = 7, 3, 1
    v.w[1, 32, 31] = 2.5
    v.eta[0] = 1e-3
    assert host[lay.r_off + 8:lay.r_off + 12].view(np.int32)[0] == 7      # views, not copies
    assert host[lay.w_off + 4 * (33 * 32 + 32 * 32 + 31):][:4].view(np.float32)[0] == 2.5
    assert host[lay.eta_off:lay.eta_off + 8].view(np.float64)[0] == 1e-3


def test_keep_tables():
    from svdq_amd.compress import keep_row
    from svdq_amd.pipeline import keep_table
    assert keep_row(["a", "b", "c", "d"], ["b", "d"]) == [1, 3]
    assert keep_row(["a", "c"], ["a", "b", "c"]) == [0, -1, 1]
    t = keep_table([2, -1, 0], 2, 3, 4)
    assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"] and t.tolist() == [[2, -1, 0], [2, -1, 0]]
    assert keep_table([[0, 1], [1, -1]], 2, 2, 2).tolist() == [[0, 1], [1, -1]]
    for bad in ([0, 1], [[0, 1, 2]], [0, 1, 4], [0, -2, 1], [0.5, 1, 2]):
        with pytest.raises(ValueError):
            keep_table(bad, 2, 3, 4)


def test_script_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import consolidate
    finally:
        sys.path.pop(0)
    ap = consolidate.build_parser()
    args = ap.parse_args(["--artifact-dir", "a"])
    assert (args.output_dir, args.tasks, args.energy_threshold, args.max_rank, args.low_bits, args.stages,
            args.min_sigma) == (None, None, None, None, None, None, 0.0)
    args = ap.parse_args(["--artifact-dir", "a", "--output-dir", "o", "--tasks", "t1", "t2", "--energy-threshold", "0.95",
                          "--max-rank", "4", "--low-bits", "8", "--stages", "3", "--min-sigma", "1e-3"])
    assert (args.output_dir, args.tasks, args.energy_threshold, args.max_rank, args.low_bits, args.stages,
            args.min_sigma) == ("o", ["t1", "t2"], 0.95, 4, 8, 3, 1e-3)
    for bad in (["--min-sigma", "small"], ["--max-rank", "2.5"], []):
        with pytest.raises(SystemExit):
            ap.parse_args((["--artifact-dir", "a"] if bad else []) + bad)


def test_value_errors_before_any_gpu_work():
    import svdq_amd
    from svdq_amd.compress import check_consolidate_room, consolidate_task_list
    comp = {"p": {"t1": {}, "t2": {}}, "q": {"t2": {}, "t3": {}}}
    assert consolidate_task_list(comp) == ["t1", "t2", "t3"]
    assert consolidate_task_list(comp, ["t3", "t1", "t3"]) == ["t1", "t3"]
    with pytest.raises(ValueError, match="not in the store"):
        consolidate_task_list(comp, ["t1", "t9"])
    with pytest.raises(ValueError, match="no task to keep"):
        consolidate_task_list(comp, [])
    with pytest.raises(ValueError, match="no task to keep"):
        consolidate_task_list({}, None)
    check_consolidate_room({"p": {"masked": _basis(100, 4, 28), "noise": None}})
    with pytest.raises(ValueError, match=r"r \+ 1 = 33 \+ 1 > 33"):
        check_consolidate_room({"p": {"masked": _basis(100, 5, 28)}})
    with pytest.raises(ValueError, match="noise"):
        check_consolidate_room({"p": {"masked": _basis(100, 1, 1), "noise": _basis(50, 30, 3)}})
    # the public entry point refuses before it looks at a tensor or a GPU
    cfg = svdq_amd.SVDHybridConfig()
    ok = {"p": {"masked": _basis(100, 4, 4), "noise": None}}
    with pytest.raises(ValueError, match="not in the store"):
        svdq_amd.consolidate_bases(comp, ok, cfg, tasks=["nope"])
    with pytest.raises(ValueError, match="no task to keep"):
        svdq_amd.consolidate_bases(comp, ok, cfg, tasks=[])
    with pytest.raises(ValueError, match=r"r \+ 1"):
        svdq_amd.consolidate_bases(comp, {"p": {"masked": _basis(100, 33, 0)}}, cfg)


def test_config_and_diagnostics_of_a_consolidated_store():
    import svdq_amd
    from svdq_amd.storage import consolidated_config, consolidated_diagnostics
    cfg = svdq_amd.SVDHybridConfig()
    assert consolidated_config(cfg) is cfg
    c2 = consolidated_config(cfg, energy_threshold=0.5, max_rank=3, low_bits=8, rtvq_stages=1, center=False)
    assert (c2.svd_energy_threshold, c2.svd_max_rank, c2.svd_low_bits, c2.svd_rtvq_stages, c2.svd_center) == \
        (0.5, 3, 8, 1, False)
    assert cfg.svd_low_bits != 8 or cfg.svd_rtvq_stages != 1      # the stored one is not touched
    with pytest.raises(ValueError):
        consolidated_config(cfg, energy_threshold=1.5)
    diag = {"per_parameter": {"p": {}}, "task_weights": {"a": 0.5, "b": 0.25, "c": 0.25}}
    res = {"columns": {("p", "masked"): (7, 2)}, "dropped_energy": {("p", "masked"): 1.5e-9}}
    out = consolidated_diagnostics(diag, ["a", "c"], res)
    assert out["task_weights"] == {"a": 0.5 / 0.75, "c": 0.25 / 0.75} and out["tasks"] == ["a", "c"]
    assert out["columns"] == {"p [masked]": [7, 2]} and out["dropped_energy"] == {"p [masked]": 1.5e-9}
    assert out["per_parameter"] == {"p": {}} and "tasks" not in diag and len(diag["task_weights"]) == 3
    assert out["promoted"] == {} and out["noise_floor"] == {}
    d2 = dict(diag, cluster_assignments={"a": 0, "b": 1, "c": 0}, captured_energy={"b": 0.5})
    o2 = consolidated_diagnostics(d2, ["a", "c"], dict(res, promoted={("p", "masked"): (2, 4)}))
    assert o2["cluster_assignments"] == {"a": 0, "c": 0} and o2["captured_energy"] == {} and len(d2["cluster_assignments"]) == 3
    assert o2["promoted"] == {"p [masked]": [2, 4]}
    assert consolidated_diagnostics({}, ["x", "y"], res)["task_weights"] == {"x": 0.5, "y": 0.5}
    sixth = {t: 1.0 / 6 for t in "abcdef"}
    assert consolidated_diagnostics({"task_weights": sixth}, list("abcdef"), res)["task_weights"] == sixth      # as stored


def test_a_c_low_the_quantizer_cannot_represent_goes_to_the_high_side():
    from svdq_amd.compress import promoted_entry, unquantizable_slots
    inf, nan = np.float32("inf"), np.float32("nan")
    scale = np.array([[3.0, 7.0], [3.0, inf], [0.0, 1.0], [2.0, 2.0], [nan, 1.0]], np.float32)
    zp = np.array([[1.0, 2.0], [1.0, nan], [1.0, 1.0], [1.0, -inf], [0.0, 0.0]], np.float32)
    assert unquantizable_slots(scale, zp, [0, 1, 2, 3]) == [1, 2, 3]
    assert unquantizable_slots(scale, zp, [0]) == [] and unquantizable_slots(scale, zp, [4, 0]) == [4]
    b = _basis(6, 2, 2, N=3)
    b["U_high"] = torch.arange(12, dtype=torch.float16).reshape(6, 2)
    b["U_low"] = -torch.arange(12, dtype=torch.float16).reshape(6, 2)
    coef = np.zeros((3, 3), np.float32)
    coef = np.arange(12, dtype=np.float32).reshape(3, 4) + 0.3
    e, arts = promoted_entry(b, coef, [0, 2])
    assert e["k"] == 4 and e["U_low"].shape == (6, 0) and e["U_low"].dtype is torch.float16 and e["energy_retained"] == 1.0
    assert torch.equal(e["U_high"], torch.cat([b["U_high"], b["U_low"]], dim=1)) and e["mean"] is b["mean"]
    assert sorted(arts) == [0, 2] and arts[2]["c_high_fp16"].dtype is torch.float16
    assert torch.equal(arts[2]["c_high_fp16"], torch.from_numpy(coef[2]).half())
    assert b["k"] == 2 and b["U_high"].shape == (6, 2)      # the input is not touched


def _tiny_store(path):
    import svdq_amd
    from svdq_amd.storage import save_all_artifacts
    q = {"payloads": [], "num_bits": 4, "num_stages": 2, "original_shape": torch.Size([0]),
         "original_dtype": "torch.float32"}
    art = lambda: {"masked": {"c_high_fp16": torch.ones(2, dtype=torch.float16), "c_low_quant": q}}
    bases = {"p": {"masked": _basis(10, 2, 0, N=2), "noise": None}}
    comp = {"p": {"t1": art(), "t2": art()}}
    diag = {"per_parameter": {"p": {}}, "task_weights": {"t1": 0.5, "t2": 0.5}}
    save_all_artifacts(bases, comp, diag, svdq_amd.SVDHybridConfig(), path)


def _snapshot(path):
    out = {}
    for root, _, files in os.walk(path):
        for f in files:
            full = os.path.join(root, f)
            out[os.path.relpath(full, path)] = open(full, "rb").read()
    return out


def test_in_place_write_goes_through_a_temporary_directory(tmp_path, monkeypatch):
    """The consolidation itself is replaced by a fixed result (no GPU here); the writer fails half way through the
    staged store: the old files are byte-identical afterwards and the staging directory is gone."""
    import svdq_amd
    from svdq_amd import compress, storage
    store = str(tmp_path / "store")
    _tiny_store(store)
    before = _snapshot(store)
    fixed = {"bases": {"p": {"masked": _basis(10, 1, 0, N=1), "noise": None}},
             "compressed": {"p": {"t1": {"masked": {"c_high_fp16": torch.zeros(1, dtype=torch.float16),
                                                    "c_low_quant": {"payloads": [], "num_bits": 4, "num_stages": 2,
                                                                    "original_shape": torch.Size([0]),
                                                                    "original_dtype": "torch.float32"}}}}},
             "columns": {("p", "masked"): (2, 1)}, "dropped_energy": {("p", "masked"): 0.0}, "skipped": []}
    monkeypatch.setattr(compress, "consolidate_bases", lambda *a, **kw: fixed)
    seen = {}
    real_save = storage.save_compressed_coefficients

    def failing(compressed, output_dir):
        seen["dir"] = output_dir
        assert os.path.exists(os.path.join(output_dir, "basis", "p.pt"))      # the staged store is half written
        raise OSError("disk full")

    monkeypatch.setattr(storage, "save_compressed_coefficients", failing)
    with pytest.raises(OSError, match="disk full"):
        storage.consolidate_artifacts(store, tasks=["t1"])
    assert os.path.realpath(seen["dir"]) != os.path.realpath(store)
    assert os.path.dirname(os.path.realpath(seen["dir"])) == os.path.dirname(os.path.realpath(store))
    assert not os.path.exists(seen["dir"])
    assert _snapshot(store) == before
    # and when nothing fails the store is rewritten: the dropped task is in no file, the bookkeeping is recorded
    monkeypatch.setattr(storage, "save_compressed_coefficients", real_save)
    res = storage.consolidate_artifacts(store, tasks=["t1"])
    assert res["tasks"] == ["t1"] and res["dropped"] == ["t2"] and res["output_dir"] == store
    art = storage.load_all_artifacts(store)
    assert list(art["compressed"]["p"].keys()) == ["t1"] and art["bases"]["p"]["masked"]["k"] == 1
    assert art["diagnostics"]["tasks"] == ["t1"] and art["diagnostics"]["task_weights"] == {"t1": 1.0}
    assert art["diagnostics"]["columns"] == {"p [masked]": [2, 1]}
    assert sorted(os.listdir(str(tmp_path))) == ["store"]
    # another output directory leaves the source alone
    now = _snapshot(store)
    res = storage.consolidate_artifacts(store, output_dir=str(tmp_path / "other"))
    assert _snapshot(store) == now and os.path.exists(str(tmp_path / "other" / "basis" / "p.pt"))
