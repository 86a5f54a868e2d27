#!/usr/bin/env python3
"""Pass 1 alone (svdq_gram_center: k_gram, or k_gram minus base with --from-base) per input dtype, timed with events.

The workload of tools/bench_input_dtype.py (the synthetic task vectors of every visual tensor of a CLIP model, built
once in fp32 and rounded once to each half dtype), one plan per dtype; the dtypes alternate, --reps rounds of
(W warm-up + K timed launches) each, every launch between two events.  Prints one JSON line: per dtype the median and
the range of the launch time in ms, the bytes pass 1 reads and GB/s at the median.  SVDQ_LIB_PATH selects the library,
so two builds are compared by alternating processes.

    python tools/bench_gram_dtype.py --tasks 8
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--dtypes", default="fp32,bf16,fp16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import svdq_amd  # noqa: F401
    from svdq_amd import workloads
    from svdq_amd.pipeline import CompressPlan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N = args.tasks
    shapes = workloads.vit_visual_shapes(args.model)
    rows = [workloads.numel(shapes[n]) for n in sorted(shapes)]
    sumD = float(sum(rows))
    bufs, _ = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    offs, tot = [], 0
    for d in rows:
        offs.append(tot)
        tot += (d + 63) // 64 * 64

    runs = {}
    for label in args.dtypes.split(","):
        dt = DTYPES[label]
        tb = [b.to(dt) for b in bufs]
        views = [[tb[t][o:o + d] for t in range(N)] for d, o in zip(rows, offs)]
        plan = CompressPlan(rows, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4,
                            rtvq_stages=2, device=dev, input_dtype=dt, gram_only=True)
        table = plan.pointer_table(views)
        plan._keep = tb
        runs[label] = {"plan": plan, "table": table, "es": torch.finfo(dt).bits // 8, "ms": []}
    torch.cuda.synchronize()

    for _ in range(args.reps):
        for r in runs.values():
            for _ in range(args.warmup):
                r["plan"].gram_center(r["table"])
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record()
                r["plan"].gram_center(r["table"])
                b.record()
            torch.cuda.synchronize()
            r["ms"] += [a.elapsed_time(b) for a, b in ev]

    out = {"tool": "bench_gram_dtype", "model": args.model, "tasks": N, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "lib": os.path.basename(os.environ.get("SVDQ_LIB_PATH", "in-tree")),
           "device": torch.cuda.get_device_name(dev), "dtypes": {}}
    for label, r in runs.items():
        gb = sumD * r["es"] * N / 1e9
        ms = statistics.median(r["ms"])
        out["dtypes"][label] = {"k_gram_ms": round(ms, 4), "min": round(min(r["ms"]), 4), "max": round(max(r["ms"]), 4),
                                "pass1_gb": round(gb, 3), "gb_per_s": round(gb / (ms / 1e3), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
