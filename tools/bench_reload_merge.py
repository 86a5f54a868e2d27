#!/usr/bin/env python3
"""What a merge from STORED artifacts costs: the per-parameter route against adoption into plans (svdq_plan_import,
driver.adopt_artifacts) followed by the batched merge -- and the import kernel against the copy ceiling.

Everything in ONE process on one GPU.

  --what merge   the bench.py workload (svdq_amd.workloads' synthetic task vectors for every visual tensor of a CLIP
                 model, or --small: the three parameters x six tasks of tests/test_hip_merge.py's reload test) goes
                 through the fused run; its dictionaries are then made PLAIN dictionaries -- what load_all_artifacts
                 returns -- with their tensors on --payloads (cuda | cpu).  Timed, host clock around a device
                 synchronise, median of --reps:
                   per_parameter_ms   merge_all_parameters on the plain dictionaries (payload upload, dequantize launch,
                                      stack and sum, reconstruct launch per parameter and task).  This is the route a
                                      commit without adopt_artifacts takes; the tool runs there too and reports only it.
                   adopt_ms           adopt_artifacts on the plain dictionaries
                   adopted_merge_ms   merge_all_parameters on the adopted dictionaries
                   resident_merge_ms  merge_all_parameters on the fused run's own dictionaries
                 and whether the three results are the same bits.
  --what kernel  svdq_plan_import alone (device events) on the artifacts of a compress step of the same workload, the
                 sources being the basis and mean of the plan that compressed; alternating in the same process with
                 svdq_hbm_probe mode 1 (copy) over the same number of bytes.  bytes = basis + mean, read and written.

    python tools/bench_reload_merge.py --what merge --tasks 8
    python tools/bench_reload_merge.py --what merge --small
    python tools/bench_reload_merge.py --what kernel --tasks 8
    python tools/bench_reload_merge.py --what kernel --tasks 20

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _to(obj, device):
    """A plain-dictionary copy (no handle into a fused run) with every tensor on ``device``, owning its elements."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().to(device).clone()
    if isinstance(obj, dict):
        return {k: _to(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and not isinstance(obj, torch.Size):
        return type(obj)(_to(v, device) for v in obj)
    return obj


def _host_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, res


def _same(a, b):
    return sorted(a) == sorted(b) and all(
        torch.equal(a[n].contiguous().view(torch.int32), b[n].contiguous().view(torch.int32)) for n in a)


def bench_merge(args, dev):
    import svdq_amd
    from svdq_amd import workloads
    N = args.tasks
    if args.small:
        N = 6
        shapes = {"enc.w1": (64, 48), "enc.b1": (64,), "enc/w2": (32, 64)}
        max_rank = 2
    else:
        shapes = workloads.vit_visual_shapes(args.model)
        max_rank = 64
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    tasks = [f"task{t:02d}" for t in range(N)]
    _, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    tv = {t: {n: views[p][j] for p, n in enumerate(names)} for j, t in enumerate(tasks)}
    cfg = svdq_amd.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=max_rank, svd_low_bits=4,
                                   svd_rtvq_stages=2)
    bases, comp = svdq_amd.run_basis_and_compress(tv, None, cfg, dev)
    where = dev if args.payloads == "cuda" else "cpu"
    plain_b = {n: {r: (_to(dict(b.items()), where) if b is not None else None) for r, b in bases[n].items()} for n in names}
    plain_c = {n: {t: {r: _to(a, where) for r, a in art.items() if a is not None} for t, art in comp[n].items()}
               for n in names}
    weights = {t: 1.0 / N for t in tasks}
    osh = {n: torch.Size(shapes[n]) for n in names}

    def merge(c, b):
        return svdq_amd.merge_all_parameters(c, b, {}, weights, osh, cfg, device=dev, verbose=False)

    out = {"tool": "bench_reload_merge", "what": "merge", "model": "three-parameter" if args.small else args.model,
           "tasks": N, "parameters": len(names), "sum_rows": int(sum(rows)), "payloads": args.payloads,
           "reps": args.reps, "device": torch.cuda.get_device_name(dev)}
    merge(plain_c, plain_b)                                    # warm-up: code objects, allocator
    slow_ms, slow = _host_ms(lambda: merge(plain_c, plain_b), args.reps)
    out["per_parameter_ms"] = {"median": round(statistics.median(slow_ms), 3), "runs": [round(x, 3) for x in slow_ms]}
    adopt = getattr(svdq_amd, "adopt_artifacts", None)
    if adopt is not None:
        adopt(plain_b, plain_c, cfg, device=dev)
        ad_ms, (ab, ac) = _host_ms(lambda: adopt(plain_b, plain_c, cfg, device=dev), args.reps)
        merge(ac, ab)
        am_ms, fast = _host_ms(lambda: merge(ac, ab), args.reps)
        merge(comp, bases)
        rm_ms, res = _host_ms(lambda: merge(comp, bases), args.reps)
        for key, ms in (("adopt_ms", ad_ms), ("adopted_merge_ms", am_ms), ("resident_merge_ms", rm_ms)):
            out[key] = {"median": round(statistics.median(ms), 3), "runs": [round(x, 3) for x in ms]}
        out["adopt_plus_merge_over_per_parameter"] = round(
            (out["adopt_ms"]["median"] + out["adopted_merge_ms"]["median"]) / out["per_parameter_ms"]["median"], 4)
        out["same_bits"] = bool(_same(fast, slow) and _same(fast, res))
    print(json.dumps(out))


def bench_kernel(args, dev):
    import ctypes
    import svdq_amd  # noqa: F401
    from svdq_amd import _native as nat, workloads
    from svdq_amd.pipeline import CompressPlan
    N = args.tasks
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    _, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    src = CompressPlan(rows, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4, rtvq_stages=2,
                       device=dev)
    src.run(src.pointer_table(views))
    sm = src.fetch_small()
    small_host = src.small.cpu().numpy()
    P = len(rows)
    uh, ul, mn = zip(*(src.basis_tensors(p, int(sm.k[p]), int(sm.r[p]), int(sm.rows[p])) for p in range(P)))
    moved = sum(int(sm.rows[p]) * (int(sm.r[p]) * 2 + 4) for p in range(P))     # basis + mean bytes, one way
    dst = CompressPlan(rows, N, center=True, fp16=True, rtvq_stages=2, device=dev, workspace=False)
    dst.import_artifacts(list(uh), list(ul), [m.reshape(-1) for m in mn], small_host)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for p in range(P)
               for a, b in zip(dst.basis_tensors(p, int(sm.k[p]), int(sm.r[p]), int(sm.rows[p])), (uh[p], ul[p], mn[p])))
    table = torch.tensor([t.data_ptr() if t.numel() else 0 for seq in (uh, ul, mn) for t in seq], dtype=torch.int64).to(dev)
    lib = nat.lib()
    vp = ctypes.c_void_p

    def run_import():
        nat.check(lib.svdq_plan_import(dst._h, vp(table.data_ptr()), vp(table.data_ptr() + 8 * P),
                                       vp(table.data_ptr() + 16 * P), vp(dst.small.data_ptr()), vp(dst.basis.data_ptr()),
                                       vp(dst.mean.data_ptr()), vp(torch.cuda.current_stream().cuda_stream)),
                  "svdq_plan_import")

    nbytes = moved // 16 * 16
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    b = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run_probe():
        nat.check(lib.svdq_hbm_probe(1, vp(a.data_ptr()), vp(b.data_ptr()), nbytes,
                                     vp(torch.cuda.current_stream().cuda_stream)), "svdq_hbm_probe")

    def event_ms(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    imp, prb = [], []
    for _ in range(args.reps):      # alternating
        imp.append(event_ms(run_import))
        prb.append(event_ms(run_probe))
    mi, mp = statistics.median(imp), statistics.median(prb)
    out = {"tool": "bench_reload_merge", "what": "kernel", "model": args.model, "tasks": N, "parameters": P,
           "units": int(dst.sizes.n_units), "steps": args.steps, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev), "bytes_one_way": moved, "copied_bits_equal": bool(same),
           "import_ms": {"median": round(mi, 4), "rounds": [round(x, 4) for x in imp]},
           "probe_copy_ms": {"median": round(mp, 4), "rounds": [round(x, 4) for x in prb]},
           "import_TBps_read_plus_write": round(2 * moved / mi / 1e9, 3),
           "probe_TBps_read_plus_write": round(2 * nbytes / mp / 1e9, 3),
           "import_over_probe_rate": round((moved / mi) / (nbytes / mp), 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("merge", "kernel"), default="merge")
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--payloads", choices=("cuda", "cpu"), default="cuda")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    (bench_merge if args.what == "merge" else bench_kernel)(args, dev)


if __name__ == "__main__":
    main()
