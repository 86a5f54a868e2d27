#!/usr/bin/env python3
"""What a Model Breadcrumbs merge of a store costs, in time and in peak memory.  Three routes in ONE process on one GPU:

  materialised  the yardstick, built only from pieces the package had before: ``reconstruct_task_vectors`` for all
                tasks, then the definition with torch on the device (two ``kthvalue``s per tensor and task)
  fused         ``merge.breadcrumbs_merge_parameters``: per digit one histogram pass (two above 16 tasks), one merge
                pass, no task model written
  ties          ``merge.ties_merge_parameters`` at density 0.2 from the same tree: the nearest existing kernel pair
                (4 histogram passes + 1 merge pass at any task count)

The bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for every visual tensor of a CLIP model;
ViT-L-14 x 8 by default) goes through ``run_basis_and_compress`` once, the task vectors are dropped, the dictionaries
stay resident.  Before any timing the fused and the materialised route are compared: both thresholds of every (parameter,
task) equal, merged values within T 2^-23 sum|v| per row (torch's reductions add in another order;
tests/test_breadcrumbs_model_cpu.py uses the same bound).  Then, alternating, a host clock around calls that end in a
device synchronise, --reps rounds of --calls calls each; ``torch.cuda.max_memory_allocated`` over the value just before
the call is recorded for one call of each route.

    python tools/bench_breadcrumbs_merge.py --out profiles/breadcrumbs_merge_vitl8.json

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_breadcrumbs_merge.py
--calls 1 --reps 1``.  Prints one JSON line (and writes it to --out).
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


def counts(D, density, gamma):
    n_keep, n_top = int(D * density), int(D * gamma)
    n_bot = D - n_keep - n_top
    if n_bot < 0:
        n_top, n_bot = n_top + n_bot, 0
    return n_keep, n_top, n_bot


def materialised(sq, comp, bases, shapes, cfg, names, tasks, density, gamma, sign_election, merge_func):
    """The definition on the N reconstructed task vectors.  Returns ({param: merged}, {param: [T, 2] thresholds})."""
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    out, bands = {}, {}
    for n in names:
        M = torch.stack([recon[t][n].reshape(-1) for t in tasks])      # [T, D_p]
        D = M.shape[1]
        n_keep, n_top, n_bot = counts(D, density, gamma)
        if n_keep == 0:
            out[n], bands[n] = torch.zeros(D, device=M.device), None
            continue
        A = M.abs()
        lo = torch.stack([A[t].kthvalue(n_bot + 1).values for t in range(M.shape[0])])
        hi = torch.stack([A[t].kthvalue(D - n_top).values for t in range(M.shape[0])])
        keep = (A >= lo.view(-1, 1)) & (A <= hi.view(-1, 1))
        if sign_election:
            positive = (M * keep).sum(dim=0) >= 0
            keep &= torch.where(positive.unsqueeze(0), M > 0, M < 0)
        merged = (M * keep).sum(dim=0)
        if merge_func == "mean":
            merged = merged / torch.clamp(keep.sum(dim=0).float(), min=1)
        out[n], bands[n] = merged, torch.stack([lo, hi], dim=1)
    return out, bands


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--density", type=float, default=0.9)
    ap.add_argument("--gamma", type=float, default=0.01)
    ap.add_argument("--sign-election", action="store_true")
    ap.add_argument("--merge-func", default="sum", choices=["mean", "sum"])
    ap.add_argument("--ties-density", type=float, default=0.2)
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
    kw = dict(density=args.density, gamma=args.gamma, sign_election=args.sign_election, merge_func=args.merge_func)

    def run_fused():
        out = sq.breadcrumbs_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True, **kw)
        torch.cuda.synchronize()
        return out

    def run_materialised():
        out = materialised(sq, comp, bases, shapes, cfg, names, tasks, **kw)
        torch.cuda.synchronize()
        return out

    def run_ties():
        out = sq.ties_merge_parameters(comp, bases, shapes, cfg, density=args.ties_density, device="cuda",
                                       return_stats=True)
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
    (mat, bands), peak_mat = peak_of(run_materialised)
    _, peak_ties = peak_of(run_ties)
    same_bands = True
    for n in names:
        for q, t in enumerate(tasks):
            got = stats["thresholds"][n][t]
            want = None if bands[n] is None else tuple(float(x) for x in bands[n][q].cpu())
            same_bands &= got == want
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
    if not (same_bands and within):
        raise SystemExit(f"the two routes disagree: thresholds equal {same_bands}, within the bound {within}, worst {worst}")
    del fused, mat, bound, err

    def wall_ms(fn):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    routes = {"fused_ms": run_fused, "materialised_ms": run_materialised, "ties_ms": run_ties}
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating; the comparison above was the warm-up of all three
        for key, fn in routes.items():
            times[key].append(wall_ms(fn))
            print(f"round {len(times[key])} {key} {times[key][-1]:.1f}", file=sys.stderr, flush=True)
    es = 2 if cfg.svd_fp16 else 4
    hist_passes = 4 if N <= 16 else 8
    plan_tables = sum({id(bases[n]["masked"]._batch[0].plan): int(
        sq._native.lib().svdq_crumbs_work_bytes(bases[n]["masked"]._batch[0].plan.P, N)) for n in names}.values())
    out = {"tool": "bench_breadcrumbs_merge", "model": args.model, "tasks": N, "parameters": len(names), "sum_rows": D,
           "mean_rank": round(r_mean, 3), "density": args.density, "gamma": args.gamma,
           "sign_election": args.sign_election, "merge_func": args.merge_func, "ties_density": args.ties_density,
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls_per_round": args.calls,
           "thresholds_equal": same_bands, "merged_within_bound": within, "worst_abs_difference": worst,
           "kept_total": stats["kept_total"], "sign_conflict_rows": stats["sign_conflict_rows"],
           "empty_rows": stats["empty_rows"], "model_bytes": 4 * D, "state_table_bytes": plan_tables,
           "peak_rise_fused_bytes": int(peak_fused), "peak_rise_materialised_bytes": int(peak_mat),
           "peak_rise_ties_bytes": int(peak_ties), "peak_rise_fused_models": round(peak_fused / (4 * D), 3),
           "peak_rise_materialised_models": round(peak_mat / (4 * D), 3),
           # every histogram pass reads basis + mean, the merge pass reads them and writes the output
           "histogram_passes": hist_passes,
           "bytes_moved_fused": int((hist_passes + 1) * D * (es * r_mean + 4) + 4 * D),
           "bytes_moved_ties": int(5 * D * (es * r_mean + 4) + 4 * D)}
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    out["materialised_over_fused"] = round(out["materialised_ms"]["median"] / out["fused_ms"]["median"], 3)
    out["fused_over_ties"] = round(out["fused_ms"]["median"] / out["ties_ms"]["median"], 3)
    out["fused_over_ties_by_bytes"] = round(out["bytes_moved_fused"] / out["bytes_moved_ties"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
