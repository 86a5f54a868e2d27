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
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of each timed window")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
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
