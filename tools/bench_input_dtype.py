#!/usr/bin/env python3
"""fp32-resident against fp16 / bf16-resident compression steps (svdq_plan_set_input_type), alternating in ONE process.

The bench.py workload -- the synthetic task vectors of svdq_amd.workloads for every visual tensor of a CLIP model --
is built once in fp32 and converted once to each half dtype (the same values rounded; outputs are therefore not
compared here: tests/test_hip_half_inputs.py checks bit identity against the half values widened to fp32).  One plan
per dtype, the same settings as bench.py's default run (energy 0.9, max_rank 64, centred, fp16 basis, 4-bit, 2 stages),
each with the same output placement policy (CompressPlan.tune_placement, --placement-candidates, before any timing).
The timed steps then alternate between the dtypes: --reps rounds of (W warm-up + K timed steps) per dtype, so drift of
the box hits every dtype alike; the median round is reported.

    python tools/bench_input_dtype.py --tasks 8                     # the plain route
    python tools/bench_input_dtype.py --tasks 8 --from-base         # fine-tuned + base tensors (svdq_compress_from_base)

Prints one JSON line: per dtype ms/step, the algorithmic GB of a step (pass 1 reads the inputs; pass 2 reads them
again and writes U in fp16 and the mean in fp32) and GB/s = GB / step time; and each half dtype's step time relative
to fp32.
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

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--from-base", action="store_true", help="fine-tuned + base tensors, delta formed in registers")
    ap.add_argument("--dtypes", default="fp32,bf16,fp16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--placement-candidates", type=int, default=6)
    args = ap.parse_args()

    import svdq_amd  # noqa: F401
    from svdq_amd import workloads
    from svdq_amd.pipeline import CompressPlan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N = args.tasks
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    sumD = float(sum(rows))
    bufs, _ = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    offs, tot = [], 0
    for d in rows:
        offs.append(tot)
        tot += (d + 63) // 64 * 64
    base = None
    if args.from_base:
        gb = torch.Generator(device=dev).manual_seed(99)
        base = torch.randn(tot, device=dev, generator=gb)
        bufs = [base + b for b in bufs]          # fine-tuned = base + delta

    runs = {}
    for label in args.dtypes.split(","):
        dt = DTYPES[label]
        tb = [b.to(dt) for b in bufs]            # one flat buffer per task (64-element aligned offsets)
        views = [[tb[t][o:o + d] for t in range(N)] for d, o in zip(rows, offs)]
        plan = CompressPlan(rows, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4,
                            rtvq_stages=2, device=dev, input_dtype=dt)
        table = plan.pointer_table(views)
        bt = bb = None
        if base is not None:
            bb = base.to(dt)
            bt = torch.tensor([bb[o:o + d].data_ptr() for d, o in zip(rows, offs)], dtype=torch.int64).to(dev)
            step = (lambda plan=plan, table=table, bt=bt: plan.run_from_base(table, bt))
        else:
            step = (lambda plan=plan, table=table: plan.run(table))
        plan._keep = (tb, bb)
        plan.tune_placement(table, candidates=args.placement_candidates)
        runs[label] = {"plan": plan, "step": step, "es": torch.finfo(dt).bits // 8, "ms": []}
    torch.cuda.synchronize()

    for _ in range(args.reps):
        for label, r in runs.items():
            for _ in range(args.warmup):
                r["step"]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                r["step"]()
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) * 1e3 / args.steps)

    out = {"tool": "bench_input_dtype", "model": args.model, "tasks": N, "route": "from_base" if base is not None else
           "plain", "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "placement_candidates": args.placement_candidates, "device": torch.cuda.get_device_name(dev), "dtypes": {}}
    for label, r in runs.items():
        es = r["es"]
        extra = 1 if base is not None else 0     # the base tensor is read beside the N fine-tuned ones
        gram = sumD * es * (N + extra)
        proj = sumD * (es * (N + extra) + 2 * N + 4)
        ms = statistics.median(r["ms"])
        out["dtypes"][label] = {"ms_per_step": round(ms, 4), "ms_rounds": [round(x, 4) for x in r["ms"]],
                                "algorithmic_gb": round((gram + proj) / 1e9, 3),
                                "pass1_gb": round(gram / 1e9, 3), "pass2_gb": round(proj / 1e9, 3),
                                "gb_per_s": round((gram + proj) / 1e9 / (ms / 1e3), 1)}
    if "fp32" in out["dtypes"]:
        f = out["dtypes"]["fp32"]["ms_per_step"]
        out["vs_fp32"] = {k: round(v["ms_per_step"] / f, 4) for k, v in out["dtypes"].items() if k != "fp32"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
