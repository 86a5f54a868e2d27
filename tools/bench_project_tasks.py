#!/usr/bin/env python3
"""What adding NEW tasks to a stored artifact set costs: compress.project_all_parameters (bases adopted into plans, one
svdq_plan_project per plan) against the per-parameter route, compress.compress_all_parameters on the same stored bases
(a selection, an svdq_project launch pair, a device-to-host copy and a quantizer call per parameter, region and task) --
and the streaming launch against the read ceiling.

Everything in ONE process on one GPU.  The store: svdq_amd.workloads' synthetic task vectors for every visual tensor of
a CLIP model, --tasks of them compressed by the fused run, its dictionaries then made PLAIN dictionaries on the GPU (what
load_all_artifacts returns); --new further task vectors from the same generator are the new tasks.  --masks: every
parameter of >= 4096 elements gets a random mask (60 % set), the store holds the masked regions.

  routes   host clock around a device synchronise, the two routes alternating, one warm-up each, --reps rounds:
             project_ms         project_all_parameters (adoption of the bases included: a new task arrives once)
             per_parameter_ms   compress_all_parameters on the same bases
  kernel   the two launches of svdq_plan_project alone (device events, --steps back to back, --reps rounds) on the
           adopted plan of the unmasked store, alternating with torch's read-only sum of a 4 GiB buffer (the read
           ceiling of tools/hbm_ceiling.py).  bytes_must_move = sum over parameters of rows * (e * r + 4 + 4 * new).

    python tools/bench_project_tasks.py --model ViT-L-14 --tasks 8 --new 1
    python tools/bench_project_tasks.py --model ViT-B-16 --tasks 8 --new 8 --masks

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
    if isinstance(obj, torch.Tensor):
        return obj.detach().to(device).clone()
    if isinstance(obj, dict):
        return {k: _to(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and not isinstance(obj, torch.Size):
        return type(obj)(_to(v, device) for v in obj)
    return obj


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def _summary(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
            "runs": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8, help="tasks of the stored set")
    ap.add_argument("--new", type=int, default=1, help="new tasks to project")
    ap.add_argument("--masks", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-routes", action="store_true", help="kernel timing only")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd
    from svdq_amd import workloads
    from svdq_amd.driver import adopt_bases

    N, M = args.tasks, args.new
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    old = [f"task{t:02d}" for t in range(N)]
    new = [f"new{t:02d}" for t in range(M)]
    _, views = workloads.synth_task_buffers(rows, N + M, seed=0, device=dev)
    tv = {t: {n: views[p][j].view(shapes[n]) for p, n in enumerate(names)} for j, t in enumerate(old + new)}
    masks = {}
    if args.masks:
        g = torch.Generator(device=dev).manual_seed(1)
        masks = {n: torch.rand(shapes[n], device=dev, generator=g) < 0.6 for n, r in zip(names, rows) if r >= 4096}
    cfg = svdq_amd.SVDHybridConfig(tasks=old, svd_energy_threshold=0.9, svd_max_rank=64, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = svdq_amd.run_basis_and_compress({t: tv[t] for t in old}, masks or None, cfg, dev)
    plain_b = {n: {r: (_to(dict(b.items()), dev) if b is not None else None) for r, b in bases[n].items()} for n in names}
    del bases, comp
    new_tv = {t: tv[t] for t in new}
    out = {"tool": "bench_project_tasks", "model": args.model, "stored_tasks": N, "new_tasks": M, "masks": bool(args.masks),
           "parameters": len(names), "sum_rows": int(sum(rows)), "reps": args.reps, "steps": args.steps,
           "device": torch.cuda.get_device_name(dev)}

    if not args.skip_routes:
        def project():
            return svdq_amd.project_all_parameters(new_tv, masks, plain_b, cfg, device=dev)

        def per_parameter():
            return svdq_amd.compress_all_parameters(new_tv, masks, plain_b, cfg, device=dev)

        a, b = project(), per_parameter()      # warm-up: code objects, allocator
        worst = 0.0
        for n in names:
            for t in new:
                x, y = a[n][t]["masked"]["c_high_fp16"].float(), b[n][t]["masked"]["c_high_fp16"].float()
                if x.numel():
                    worst = max(worst, float(((x - y).abs() / (y.abs() + 1e-6)).max()))
        out["c_high_worst_rel_diff_between_routes"] = worst
        pm, sm_ = [], []
        for _ in range(args.reps):             # alternating
            pm.append(_host_ms(project)[0])
            sm_.append(_host_ms(per_parameter)[0])
        out["project_ms"], out["per_parameter_ms"] = _summary(pm), _summary(sm_)
        out["per_parameter_over_project"] = round(out["per_parameter_ms"]["median"] / out["project_ms"]["median"], 3)
        del a, b

    if not args.masks:
        batches, declined = adopt_bases(plain_b, cfg, M, device=dev)
        assert len(batches) == 1 and not declined, (len(batches), declined)
        batch = batches[0]
        plan = batch.plan
        tab = [0] * (plan.P * plan.N)
        keep = []
        for i, (name, _) in enumerate(batch.entries):
            for j, t in enumerate(new):
                v = new_tv[t][name].reshape(-1)
                keep.append(v)
                tab[i * plan.N + j] = v.data_ptr()
        table = torch.tensor(tab, dtype=torch.int64).to(dev)
        must = sum(int(batch.small.rows[i]) * (2 * int(batch.small.r[i]) + 4 + 4 * M) for i in range(plan.P))
        x = torch.randn(1 << 30, device=dev)

        def event_ms(fn, steps):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / steps

        km, rm = [], []
        for _ in range(args.reps):             # alternating
            km.append(event_ms(lambda: plan.project_tasks(table, fetch=False), args.steps))
            rm.append(event_ms(lambda: x.sum(), args.steps))
        k, r = statistics.median(km), statistics.median(rm)
        ceiling = 4 * x.numel() / r / 1e9
        out.update({"plan_tasks": plan.N, "units": int(plan.sizes.n_units), "bytes_must_move": must,
                    "kernel_ms": _summary(km), "read_4GiB_ms": _summary(rm),
                    "kernel_TBps": round(must / k / 1e9, 3), "read_ceiling_TBps": round(ceiling, 3),
                    "share_of_read_ceiling": round(must / k / 1e9 / ceiling, 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
