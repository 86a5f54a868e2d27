#!/usr/bin/env python3
"""What the task Gram costs a cluster-weighted run: a third pass over the deltas against a by-product of pass 1.

The bench.py workload -- the synthetic task vectors of svdq_amd.workloads for every visual tensor of a CLIP model --
in ONE process, the two arms alternating:

  (a) compress on a plan without the by-product, then svdq_task_gram on a gram_only plan over the same tensors
      (what a cluster-weighted run did before: the deltas are read three times);
  (b) compress on a plan with the by-product (CompressPlan(task_gram=True)), then svdq_plan_task_gram.

Same settings as bench.py's default run (energy 0.9, max_rank 64, centred, fp16 basis, 4-bit, 2 stages) and the same
output placement policy for both compressing plans (CompressPlan.tune_placement, before any timing).  --reps rounds of
(W warm-up + K timed steps) per arm; the median round is reported.  Besides the steps, pass 1 alone (gram_center on
either plan), svdq_task_gram alone and svdq_plan_task_gram alone are timed with device events, which is the
per-kernel split the comparison needs: the by-product pays when pass1(b) - pass1(a) + plan_task_gram < task_gram.

    python tools/bench_task_gram.py --tasks 8
    python tools/bench_task_gram.py --tasks 20

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


def _event_ms(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
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
    bufs, _ = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    offs, tot = [], 0
    for d in rows:
        offs.append(tot)
        tot += (d + 63) // 64 * 64
    views = [[bufs[t][o:o + d] for t in range(N)] for d, o in zip(rows, offs)]

    def compressing(task_gram):
        plan = CompressPlan(rows, N, energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4,
                            rtvq_stages=2, device=dev, task_gram=task_gram)
        table = plan.pointer_table(views)
        plan.tune_placement(table, candidates=args.placement_candidates)
        return plan, table

    plan_a, table_a = compressing(False)
    plan_b, table_b = compressing(True)
    gplan = CompressPlan(rows, N, center=False, device=dev, gram_only=True)
    gtable = gplan.pointer_table(views)

    def step_a():
        plan_a.run(table_a)
        return gplan.task_gram(gtable)

    def step_b():
        plan_b.run(table_b)
        return plan_b.compress_task_gram()

    Ga, Gb = step_a(), step_b()
    torch.cuda.synchronize()
    scale = float(Ga.abs().max())
    max_diff = float((Ga - Gb).abs().max())

    arms = {"a_compress_then_task_gram": {"step": step_a, "ms": []},
            "b_compress_with_byproduct": {"step": step_b, "ms": []}}
    split = {"pass1_plain": [], "pass1_byproduct": [], "task_gram": [], "plan_task_gram": []}
    for _ in range(args.reps):
        for r in arms.values():
            for _ in range(args.warmup):
                r["step"]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                r["step"]()
            torch.cuda.synchronize()
            r["ms"].append((time.perf_counter() - t0) * 1e3 / args.steps)
        split["pass1_plain"].append(_event_ms(lambda: plan_a.gram_center(table_a), args.steps))
        split["pass1_byproduct"].append(_event_ms(lambda: plan_b.gram_center(table_b), args.steps))
        split["task_gram"].append(_event_ms(lambda: gplan.task_gram(gtable), args.steps))
        plan_b.run(table_b)     # svdq_plan_task_gram needs the eigen stage's reduced partials of a whole run
        split["plan_task_gram"].append(_event_ms(plan_b.compress_task_gram, args.steps))

    med = {k: statistics.median(v) for k, v in split.items()}
    out = {"tool": "bench_task_gram", "model": args.model, "tasks": N, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "placement_candidates": args.placement_candidates,
           "device": torch.cuda.get_device_name(dev), "sum_rows": int(sum(rows)),
           "gram_max_abs_diff_over_max": max_diff / scale if scale else 0.0, "arms": {}, "kernels_ms": {}}
    for label, r in arms.items():
        out["arms"][label] = {"ms_per_step": round(statistics.median(r["ms"]), 4),
                              "ms_rounds": [round(x, 4) for x in r["ms"]]}
    for k, v in split.items():
        out["kernels_ms"][k] = {"median": round(med[k], 4), "rounds": [round(x, 4) for x in v]}
    a = out["arms"]["a_compress_then_task_gram"]["ms_per_step"]
    b = out["arms"]["b_compress_with_byproduct"]["ms_per_step"]
    out["b_over_a"] = round(b / a, 4)
    out["byproduct_cost_ms"] = round(med["pass1_byproduct"] - med["pass1_plain"] + med["plan_task_gram"], 4)
    out["replaces_ms"] = round(med["task_gram"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
