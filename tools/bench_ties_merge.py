#!/usr/bin/env python3
"""What a TIES merge of a store costs, in time and in peak memory: the fused route (merge.ties_merge_parameters: four
histogram passes and one merge pass over the basis, no task model written) against the materialised route built only
from pieces the package had before -- ``reconstruct_task_vectors`` for all tasks, then the published steps
(topk_values_mask / resolve_sign / disjoint_merge) with torch on the device.  The materialised route is the yardstick.

Everything in ONE process on one GPU: the bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for
every visual tensor of a CLIP model; ViT-L-14 x 8 by default) goes through ``run_basis_and_compress`` once, the task
vectors are dropped, the dictionaries stay resident.  Before any timing the two routes are compared: thresholds equal,
merged values within T 2^-23 sum|v| per row (torch's reductions add in another order; tests/test_ties_model_cpu.py has
the argument).  Then, alternating, a host clock around calls that end in a device synchronise (the host's table building
is part of what a caller pays), --reps rounds of --calls calls each; ``torch.cuda.max_memory_allocated`` over the value
just before the call is recorded for one call of each route.

    python tools/bench_ties_merge.py --out profiles/ties_merge_vitl8.json

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_ties_merge.py --calls 1
--reps 1``.  Prints one JSON line (and writes it to --out).
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


def materialised(sq, comp, bases, shapes, cfg, names, tasks, density, merge_func):
    """The published steps on the N reconstructed task vectors.  Returns ({param: merged}, thresholds [T])."""
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    M = torch.stack([torch.cat([recon[t][n].reshape(-1) for n in names]) for t in tasks])      # [T, D]
    del recon
    D = M.shape[1]
    j = max(D - int(D * density), 1)
    tau = torch.stack([M[t].abs().kthvalue(j).values for t in range(M.shape[0])])
    M = M * (M.abs() >= tau.view(-1, 1))
    sign = torch.sign(M.sum(dim=0))
    sign[sign == 0] = 1
    M = M * torch.where(sign.unsqueeze(0) > 0, M > 0, M < 0)
    merged = M.sum(dim=0)
    if merge_func == "mean":
        merged = merged / torch.clamp((M != 0).sum(dim=0).float(), min=1)
    out, off = {}, 0
    for n in names:
        out[n] = merged[off:off + shapes[n].numel()]
        off += shapes[n].numel()
    return out, tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--merge-func", default="mean", choices=["mean", "sum"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed round and route")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd as sq
    from svdq_amd import workloads
    N = args.tasks
    vshapes = workloads.vit_visual_shapes(args.model)
    names = sorted(vshapes)
    rows = [workloads.numel(vshapes[n]) for n in names]
    tasks = [f"t{i:02d}" for i in range(N)]
    keep, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    tv = {t: {n: views[p][q] for p, n in enumerate(names)} for q, t in enumerate(tasks)}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=64, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    del keep, views, tv
    torch.cuda.empty_cache()
    shapes = {n: torch.Size([r]) for n, r in zip(names, rows)}
    D = sum(rows)
    r_mean = sum(int(bases[n]["masked"]["k"] + bases[n]["masked"]["U_low"].shape[1]) * r for n, r in zip(names, rows)) / D

    def run_fused():
        out = sq.ties_merge_parameters(comp, bases, shapes, cfg, density=args.density, merge_func=args.merge_func,
                                       device="cuda", return_stats=True)
        torch.cuda.synchronize()
        return out

    def run_materialised():
        out = materialised(sq, comp, bases, shapes, cfg, names, tasks, args.density, args.merge_func)
        torch.cuda.synchronize()
        return out

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        res = fn()
        return res, torch.cuda.max_memory_allocated() - before

    (fused, stats), peak_fused = peak_of(run_fused)
    (mat, tau), peak_mat = peak_of(run_materialised)
    tau_fused = torch.tensor([stats["thresholds"][t] for t in tasks])
    same_tau = bool(torch.equal(tau_fused, tau.cpu()))
    # the bound needs sum|v| per row: one more reconstruction, task by task
    bound = torch.zeros(D, device=dev, dtype=torch.float64)
    for t in tasks:
        rec = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[t], device="cuda")[t]
        bound += torch.cat([rec[n].reshape(-1) for n in names]).abs().double()
        del rec
    bound *= N * 2.0 ** -23
    err = (torch.cat([fused[n].reshape(-1) for n in names]).double() - torch.cat([mat[n] for n in names]).double()).abs()
    within = bool((err <= bound).all())
    worst = float(err.max())
    if not (same_tau and within):
        raise SystemExit(f"the two routes disagree: thresholds equal {same_tau}, within the bound {within}, worst {worst}")
    del fused, mat, bound, err

    def wall_ms(fn):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    routes = {"fused_ms": run_fused, "materialised_ms": run_materialised}
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating; the comparison above was the warm-up of both
        for key, fn in routes.items():
            times[key].append(wall_ms(fn))
    es = 2 if cfg.svd_fp16 else 4
    out = {"tool": "bench_ties_merge", "model": args.model, "tasks": N, "parameters": len(names), "sum_rows": D,
           "mean_rank": round(r_mean, 3), "density": args.density, "merge_func": args.merge_func,
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls_per_round": args.calls,
           "thresholds_equal": same_tau, "merged_within_bound": within, "worst_abs_difference": worst,
           "kept": stats["kept"], "sign_conflict_rows": stats["sign_conflict_rows"], "empty_rows": stats["empty_rows"],
           "model_bytes": 4 * D, "peak_rise_fused_bytes": int(peak_fused), "peak_rise_materialised_bytes": int(peak_mat),
           "peak_rise_fused_models": round(peak_fused / (4 * D), 3),
           "peak_rise_materialised_models": round(peak_mat / (4 * D), 3),
           # four histogram passes read basis + mean, the merge pass reads them and writes the output
           "bytes_moved_fused": int(5 * D * (es * r_mean + 4) + 4 * D)}
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    out["materialised_over_fused"] = round(out["materialised_ms"]["median"] / out["fused_ms"]["median"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
