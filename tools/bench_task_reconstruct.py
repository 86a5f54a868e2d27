#!/usr/bin/env python3
"""What getting EVERY task's model back out of a plan costs: N merges with one-hot weights (the best plan-level route
without svdq_task_reconstruct: N passes over the basis) against ONE CompressPlan.reconstruct_tasks (one pass, N outputs).

Everything in ONE process on one GPU: the bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for
every visual tensor of a CLIP model) is compressed once, the artifacts stay resident, ``base`` is given.  Before any
timing the two routes' outputs are compared bit for bit (the tool fails otherwise).  Then, alternating, device events
around --seconds worth of back-to-back calls each, --reps rounds:
    (a) merges_ms        N x plan.merge, one-hot [1, N] weights, into N buffers
    (b) reconstruct_ms   one plan.reconstruct_tasks into the same N buffers
    (c) probe_copy_ms    svdq_hbm_probe mode 1 (copy) over as many bytes as (b) moves: the copy ceiling of this box
bytes moved by (b), from shapes and the ranks in the small buffer: sum_p rows_p (e r_p + 4 [center] + 4 [base] + 4 N).

    python tools/bench_task_reconstruct.py --tasks 8
    python tools/bench_task_reconstruct.py --tasks 16
    python tools/bench_task_reconstruct.py --tasks 20

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_task_reconstruct.py ...``.
Prints one JSON line.

``--masks union [--noise]``: the MASKED run at the dictionary level (bench.py --masks union's masks: per-task rand > 0.7
from seed 77, combined by union; ViT-B-16 x 8 unless told otherwise).  One fused run through ``run_basis_and_compress``,
then every task's model, tensors on the device, ``base_state_dict=base`` -- ``reconstruct_task_vectors`` (compacted rows, a
scatter per (parameter, task), ``base +`` afterwards) against ``reconstruct_task_vectors_masked`` (``fused_masks``: one
svdq_task_reconstruct_masked per plan), compared bit for bit, then timed alternating by a host clock around calls that end
in a device synchronise (the host's table building is part of what a caller pays).  In a checkout that has no
``reconstruct_task_vectors_masked`` only the first column is timed (the parent commit's figure).  ``--kernel-pair``: instead of timing,
a few fused calls and a few masked merges (``merge_all_parameters``: k_merge_expand<., 1, .>) on the same plans, and the
bytes each kernel moves per call -- the run to put under rocprofv3.

    python tools/bench_task_reconstruct.py --masks union --noise
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_task_reconstruct.py --masks union --noise --kernel-pair
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def masked_main(args, dev):
    """--masks union: every task's model of a masked fused run, compacted route against fused_masks."""
    import svdq_amd as sq
    from svdq_amd import workloads
    N = args.tasks
    model = args.model or "ViT-B-16"
    shapes = workloads.vit_visual_shapes(model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    tasks = [f"t{i:02d}" for i in range(N)]
    keep, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    tv = {t: {n: views[p][q] for p, n in enumerate(names)} for q, t in enumerate(tasks)}
    # bench.py --masks union's masks: one draw per task over the concatenated parameters, 64-byte aligned slices
    gm = torch.Generator(device=dev).manual_seed(77)
    offs, tot = [], 0
    for r in rows:
        offs.append(tot)
        tot += (r + 63) // 64 * 64
    union = torch.zeros(tot, dtype=torch.bool, device=dev)
    for _ in range(N):
        union |= torch.rand(tot, device=dev, generator=gm) > 0.7
    masks = {n: union[o:o + r] for n, o, r in zip(names, offs, rows)}
    cfg = sq.SVDHybridConfig(tasks=tasks, svd_energy_threshold=0.9, svd_max_rank=64, svd_low_bits=4, svd_rtvq_stages=2,
                             svd_include_noise=bool(args.noise), svd_noise_shrink=0.5)
    bases, comp = sq.run_basis_and_compress(tv, masks, cfg, "cuda")
    flat_shapes = {n: torch.Size([r]) for n, r in zip(names, rows)}
    g = torch.Generator(device=dev).manual_seed(1)
    base = {n: torch.randn(r, generator=g, device=dev) for n, r in zip(names, rows)}
    has_kw = hasattr(sq, "reconstruct_task_vectors_masked")

    def run(fused):
        fn = sq.reconstruct_task_vectors_masked if fused else sq.reconstruct_task_vectors
        out = fn(comp, bases, masks, flat_shapes, cfg, device="cuda", base_state_dict=base)
        torch.cuda.synchronize()
        return out

    # what the two source-walk kernels move per call, from shapes and the ranks in the small buffers
    regions = ("masked", "noise") if args.noise else ("masked",)
    sel_rows = src_rows = 0
    bytes_task = bytes_merge = 0
    plans = set()
    for n in names:
        live_noise = args.noise and bases[n].get("noise") is not None
        for region in regions:
            e = bases[n].get(region)
            if e is None:
                continue
            batch, i = e._batch
            plans.add(id(batch.plan))
            S, D, r = int(batch.plan.rows[i]), int(batch.small.rows[i]), int(batch.small.r[i])
            es = 2 if batch.plan.fp16 else 4
            written = S if (region == "masked" and not live_noise) else D
            sel_rows, src_rows = sel_rows + D, src_rows + S
            bytes_task += S * 5 + written * 4 * N + D * (es * r + 4)
            bytes_merge += S * 5 + written * 4 + D * (es * r + 4)
    out = {"tool": "bench_task_reconstruct", "mode": "masks", "model": model, "tasks": N, "parameters": len(names),
           "plans": len(plans), "noise": bool(args.noise), "sum_rows": int(sum(rows)), "source_rows_walked": src_rows,
           "selected_rows": sel_rows, "mask_density": round(float(union.sum()) / tot, 4),
           "device": torch.cuda.get_device_name(dev), "has_fused_masks": has_kw,
           "bytes_k_task_expand": bytes_task, "bytes_k_merge_expand": bytes_merge}
    a = run(False)
    if has_kw:
        b = run(True)
        same = all(torch.equal(a[t][n].view(torch.int32), b[t][n].view(torch.int32)) for t in tasks for n in names)
        if not same:
            raise SystemExit("reconstruct_task_vectors_masked and the compacted route differ in bits")
        out["same_bits"] = True
        out["tasks_differ"] = not torch.equal(b[tasks[0]][names[-1]], b[tasks[1]][names[-1]])
        del b
    del a
    if args.kernel_pair:
        weights = {t: 1.0 / N for t in tasks}
        for _ in range(5):
            if has_kw:
                run(True)
            sq.merge_all_parameters(comp, bases, masks, weights, flat_shapes, cfg, device="cuda", verbose=False)
            torch.cuda.synchronize()
        out["kernel_pair_calls"] = 5
        print(json.dumps(out))
        return

    def wall_ms(fused, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            run(fused)
        return (time.perf_counter() - t0) * 1e3 / calls

    routes = {"compacted_ms": False}
    if has_kw:
        routes["fused_ms"] = True
    calls = {}
    for key, fused in routes.items():      # warm-up, and how many calls fill the window
        wall_ms(fused, 2)
        calls[key] = max(2, math.ceil(args.seconds * 1e3 / wall_ms(fused, 2)))
    times = {key: [] for key in routes}
    for _ in range(args.reps):             # alternating
        for key, fused in routes.items():
            times[key].append(wall_ms(fused, calls[key]))
    out.update(reps=args.reps, window_s=args.seconds, calls=calls)
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    if has_kw:
        out["compacted_over_fused"] = round(out["compacted_ms"]["median"] / out["fused_ms"]["median"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=None, help="default: ViT-L-14, with --masks ViT-B-16")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of each timed window")
    ap.add_argument("--masks", choices=("none", "union"), default="none")
    ap.add_argument("--noise", action="store_true", help="with --masks: noise regions too (svd_include_noise)")
    ap.add_argument("--kernel-pair", action="store_true",
                    help="with --masks: no timing; k_task_expand and k_merge_expand on the same plans, for rocprofv3")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.masks != "none":
        return masked_main(args, dev)
    if args.noise or args.kernel_pair:
        ap.error("--noise and --kernel-pair need --masks union")
    args.model = args.model or "ViT-L-14"
    import svdq_amd  # noqa: F401
    from svdq_amd import _native as nat, workloads
    from svdq_amd.pipeline import CompressPlan
    N = args.tasks
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    P = len(rows)
    keep, views = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    plan = CompressPlan(rows, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4, rtvq_stages=2,
                        device=dev)
    plan.run(plan.pointer_table(views))
    sm = plan.fetch_small()
    plan._keep = None
    del keep, views
    torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(1)
    base = [torch.randn(r, generator=g, device=dev) for r in rows]
    base_table = torch.tensor([b.data_ptr() for b in base], dtype=torch.int64).to(dev)
    moved = sum(int(sm.rows[p]) * (2 * int(sm.r[p]) + 4 + 4 + 4 * N) for p in range(P))
    r_mean = sum(int(sm.rows[p]) * int(sm.r[p]) for p in range(P)) / max(sum(int(sm.rows[p]) for p in range(P)), 1)

    one_hot = []
    for t in range(N):
        w = torch.full((1, N), -1.0)
        w[0, t] = 1.0
        one_hot.append(w.to(dev))
    outs_a = [plan.new_merged_outputs() for _ in range(N)]
    outs_b = [plan.new_merged_outputs() for _ in range(N)]
    table_b = torch.stack([tab for _, _, tab in outs_b], dim=1).contiguous()      # [P, N]
    idx = torch.arange(N, dtype=torch.int32, device=dev)

    def run_merges():
        for t in range(N):
            plan.merge(one_hot[t], base_table=base_table, out_table=outs_a[t][2])

    def run_reconstruct():
        plan.reconstruct_tasks(idx, table_b, base_table=base_table)

    nbytes = moved // 2 // 16 * 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lib, vp = nat.lib(), ctypes.c_void_p

    def run_probe():
        nat.check(lib.svdq_hbm_probe(1, vp(src.data_ptr()), vp(dst.data_ptr()), nbytes,
                                     vp(torch.cuda.current_stream().cuda_stream)), "svdq_hbm_probe")

    run_merges()
    run_reconstruct()
    torch.cuda.synchronize()
    same = all(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) for a, b in zip(outs_a, outs_b))
    if not same:
        raise SystemExit("the N one-hot merges and reconstruct_tasks differ in bits")
    differ = N == 1 or not torch.equal(outs_b[0][0], outs_b[1][0])

    def event_ms(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    routes = {"merges_ms": run_merges, "reconstruct_ms": run_reconstruct, "probe_copy_ms": run_probe}
    steps = {}
    for key, fn in routes.items():      # warm-up, and how many calls fill the window
        event_ms(fn, 3)
        steps[key] = max(3, math.ceil(args.seconds * 1e3 / event_ms(fn, 5)))
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating
        for key, fn in routes.items():
            times[key].append(event_ms(fn, steps[key]))
    med = {key: statistics.median(v) for key, v in times.items()}
    out = {"tool": "bench_task_reconstruct", "model": args.model, "tasks": N, "parameters": P,
           "units": int(plan.sizes.n_units), "sum_rows": int(sum(rows)), "mean_rank": round(r_mean, 3),
           "reps": args.reps, "window_s": args.seconds, "steps": steps, "device": torch.cuda.get_device_name(dev),
           "same_bits": bool(same), "tasks_differ": bool(differ), "bytes_moved_reconstruct": moved}
    for key in routes:
        out[key] = {"median": round(med[key], 4), "rounds": [round(x, 4) for x in times[key]]}
    out["merges_over_reconstruct"] = round(med["merges_ms"] / med["reconstruct_ms"], 3)
    out["reconstruct_TBps"] = round(moved / med["reconstruct_ms"] / 1e9, 3)
    out["probe_copy_TBps_read_plus_write"] = round(2 * nbytes / med["probe_copy_ms"] / 1e9, 3)
    out["reconstruct_over_probe_rate"] = round((moved / med["reconstruct_ms"]) / (2 * nbytes / med["probe_copy_ms"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
