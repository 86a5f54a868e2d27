#!/usr/bin/env python3
"""What a DARE merge of a store costs, in time and in peak memory: the fused route (merge.dare_merge_parameters: one pass
over the basis, no task model written) against the materialised route built only from pieces the package had before --
``reconstruct_task_vectors`` for all tasks, then ``torch.bernoulli``, the division and the weighted stacked sum on the
device.  The materialised route is the yardstick.  The fused route is also timed at drop rate 0 (task arithmetic: the
generator is skipped), so the difference to the drop rate asked for is what the generator costs.

Everything in ONE process on one GPU: the bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for
every visual tensor of a CLIP model; ViT-L-14 x 8 by default) goes through ``run_basis_and_compress`` once, the task
vectors are dropped, the dictionaries stay resident.  Before any timing the routes are compared where they can be: the
two generators differ, so the merged values are compared at drop rate 0 (within T 2^-23 sum|w v| per row: torch's
reduction adds in another order), and the fused route's kept counts at the drop rate asked for must lie within six
binomial standard deviations of D (1 - p).  Then, alternating, a host clock around calls that end in a device
synchronise (the host's table building is part of what a caller pays), --reps rounds of --calls calls each;
``torch.cuda.max_memory_allocated`` over the value just before the call is recorded for one call of each route.

    python tools/bench_dare_merge.py --out profiles/dare_merge_vitl8.json
    python tools/bench_dare_merge.py --tasks 20 --out profiles/dare_merge_vitl20.json

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_dare_merge.py --calls 1
--reps 1``.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def materialised(sq, comp, bases, shapes, cfg, names, tasks, drop_rate, weights):
    """Drop, rescale and add on the N reconstructed task vectors.  Returns {param: merged}."""
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    M = torch.stack([torch.cat([recon[t][n].reshape(-1) for n in names]) for t in tasks])      # [T, D]
    del recon
    if drop_rate > 0:
        M = M * torch.bernoulli(torch.full_like(M, 1.0 - drop_rate))
        M = M / (1.0 - drop_rate)
    merged = (M * weights.view(-1, 1)).sum(dim=0)
    out, off = {}, 0
    for n in names:
        out[n] = merged[off:off + shapes[n].numel()]
        off += shapes[n].numel()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--drop-rate", type=float, default=0.9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed round and route")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd as sq
    from svdq_amd import workloads
    N, p = args.tasks, args.drop_rate
    vshapes = workloads.vit_visual_shapes(args.model)
    names = sorted(vshapes)
    rows = [workloads.numel(vshapes[n]) for n in names]
    tasks = [f"t{i:02d}" for i in range(N)]
    keep, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    tv = {t: {n: views[pi][q] for pi, n in enumerate(names)} for q, t in enumerate(tasks)}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=64, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = sq.run_basis_and_compress(tv, None, cfg, "cuda")
    del keep, views, tv
    torch.cuda.empty_cache()
    shapes = {n: torch.Size([r]) for n, r in zip(names, rows)}
    D = sum(rows)
    r_mean = sum(int(bases[n]["masked"]["k"] + bases[n]["masked"]["U_low"].shape[1]) * r for n, r in zip(names, rows)) / D
    w_host = {t: 1.0 for t in tasks}
    w_dev = torch.ones(N, device=dev)

    def run_fused(drop_rate=p):
        out = sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=drop_rate, seed=args.seed, weights=w_host,
                                       device="cuda", return_stats=True)
        torch.cuda.synchronize()
        return out

    def run_fused_zero():
        return run_fused(0.0)

    def run_materialised(drop_rate=p):
        out = materialised(sq, comp, bases, shapes, cfg, names, tasks, drop_rate, w_dev)
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
    del fused
    mat, peak_mat = peak_of(run_materialised)
    del mat
    sd = math.sqrt(D * p * (1.0 - p))
    kept_ok = all(abs(c - D * (1.0 - p)) <= 6 * sd for c in stats["kept"].values()) if p > 0 else True
    # drop rate 0: the routes compute the same sum in another order
    fused0, stats0 = run_fused_zero()
    mat0 = run_materialised(0.0)
    bound = torch.zeros(D, device=dev, dtype=torch.float64)
    for t in tasks:
        rec = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[t], device="cuda")[t]
        bound += torch.cat([rec[n].reshape(-1) for n in names]).abs().double()
        del rec
    bound *= N * 2.0 ** -23
    err = (torch.cat([fused0[n].reshape(-1) for n in names]).double() - torch.cat([mat0[n] for n in names]).double()).abs()
    within = bool((err <= bound).all())
    worst = float(err.max())
    all_kept = all(c == D for c in stats0["kept"].values())
    if not (kept_ok and within and all_kept):
        raise SystemExit(f"the routes disagree: kept counts within six sigma {kept_ok}, every value kept at drop rate 0 "
                         f"{all_kept}, sums at drop rate 0 within the bound {within} (worst {worst})")
    del fused0, mat0, bound, err
    torch.cuda.empty_cache()

    def wall_ms(fn):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    routes = {"fused_ms": run_fused, "fused_drop0_ms": run_fused_zero, "materialised_ms": run_materialised}
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating; the comparison above was the warm-up of all three
        for key, fn in routes.items():
            times[key].append(wall_ms(fn))
    es = 2 if cfg.svd_fp16 else 4
    out = {"tool": "bench_dare_merge", "model": args.model, "tasks": N, "parameters": len(names), "sum_rows": D,
           "mean_rank": round(r_mean, 3), "drop_rate": p, "drop_threshold": stats["drop_threshold"], "seed": args.seed,
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "calls_per_round": args.calls,
           "kept_within_six_sigma": kept_ok, "drop0_sums_within_bound": within, "drop0_worst_abs_difference": worst,
           "kept": stats["kept"], "model_bytes": 4 * D, "peak_rise_fused_bytes": int(peak_fused),
           "peak_rise_materialised_bytes": int(peak_mat), "peak_rise_fused_models": round(peak_fused / (4 * D), 3),
           "peak_rise_materialised_models": round(peak_mat / (4 * D), 3),
           # one pass: reads basis + mean, writes the output
           "bytes_moved_fused": int(D * (es * r_mean + 4) + 4 * D)}
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    out["generator_ms"] = round(out["fused_ms"]["median"] - out["fused_drop0_ms"]["median"], 3)
    out["materialised_over_fused"] = round(out["materialised_ms"]["median"] / out["fused_ms"]["median"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
