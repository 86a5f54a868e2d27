#!/usr/bin/env python3
"""What the task Gram of a STORE costs: svdq_plan_store_gram (CompressPlan.store_gram: one pass over the stored basis and
mean) against the only route there was before it -- every task's model reconstructed (svdq_task_reconstruct for all N
tasks) and svdq_task_gram over the N outputs -- and against the read rate of the box.

Everything in ONE process on one GPU.  The store is the tool's own: for every visual tensor of a CLIP model a random
fp16 basis [rows, r = N] (k = N / 4 high columns), a random fp32 mean and random 4-bit two-stage codes, adopted into one
centred plan by svdq_plan_import.  Device events around --steps back-to-back calls, --rounds rounds, the three arms
alternating inside a round, medians reported:

    reconstruct_gram_ms   (a) reconstruct_tasks for all N tasks, then task_gram over the outputs
                          traffic model: rows * (2 r + 4) read + rows * 4 N written + rows * 4 N read = 84 B/row at N = r = 8
    store_gram_ms         (b) store_gram: rows * (2 r + 4) read = 20 B/row at N = r = 8
    probe_ms              svdq_hbm_probe mode 0 (read only) over as many bytes as (b) reads

    python tools/bench_store_gram.py --model ViT-L-14 --tasks 8
    python tools/bench_store_gram.py --model ViT-L-14 --tasks 20

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "runs": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from ctypes import c_void_p
    from svdq_amd import _native as nat, workloads
    from svdq_amd.pipeline import CompressPlan, _stream_ptr, pack_small

    N, S = args.tasks, 2
    r, k = N, max(1, N // 4)
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    P = len(rows)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    plan = CompressPlan(rows, N, center=True, fp16=True, low_bits=4, rtvq_stages=S, device=dev, workspace=False)
    uh, ul, mn, entries = [], [], [], []
    for D in rows:
        rr, kk = min(r, D), min(k, min(r, D))
        u = (torch.randn(D, rr, device=dev, generator=g) / np.sqrt(D)).half()
        uh.append(u[:, :kk].contiguous())
        ul.append(u[:, kk:].contiguous())
        mn.append(torch.randn(D, device=dev, generator=g) / np.sqrt(D))
        entries.append({"rows": D, "k": kk, "r": rr, "energy": 0.9, "sigma": np.ones(rr, np.float32),
                        "c_high": rng.standard_normal((N, kk)).astype(np.float16),
                        "codes": rng.integers(0, 16, (N, S, rr - kk)).astype(np.uint8),
                        "scale": rng.uniform(2.0, 32.0, (N, S)).astype(np.float32),
                        "zero_point": rng.integers(0, 16, (N, S)).astype(np.float32),
                        "residual_norm": np.zeros((N, S), np.float32)})
    plan.import_artifacts(uh, ul, mn, pack_small(plan.layout, P, N, S, entries))
    torch.cuda.synchronize()
    del uh, ul, mn
    torch.cuda.empty_cache()
    sum_rows = int(sum(rows))
    read_bytes = sum(D * (2 * e["r"] + 4) for D, e in zip(rows, entries))

    # (a) every task's reconstruction into one buffer, then the Gram of the N outputs
    offs, tot = [], 0
    for D in rows:
        offs.append(tot)
        tot += (D + 63) // 64 * 64
    outbuf = torch.empty(N * tot, dtype=torch.float32, device=dev)
    out_tab = torch.tensor([[outbuf.data_ptr() + 4 * (t * tot + offs[p]) for t in range(N)] for p in range(P)],
                           dtype=torch.int64).to(dev)
    gplan = CompressPlan(rows, N, center=False, device=dev, gram_only=True)
    gram_tab = out_tab.reshape(-1).contiguous()      # [P * N] parameter-major: the same pointers

    def arm_a():
        plan.reconstruct_tasks(list(range(N)), out_tab)
        return gplan.task_gram(gram_tab)

    def arm_b():
        return plan.store_gram()

    lib = nat.lib()
    src = torch.empty(read_bytes, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty(read_bytes, dtype=torch.uint8, device=dev)

    def probe():
        nat.check(lib.svdq_hbm_probe(0, c_void_p(src.data_ptr()), c_void_p(dst.data_ptr()), read_bytes, _stream_ptr()),
                  "svdq_hbm_probe")

    def event_ms(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    Ga, Gb = arm_a(), arm_b().sum(dim=0)      # warm-up: code objects, work buffers, allocator
    probe()
    torch.cuda.synchronize()
    rel = float((Ga - Gb).abs().max() / Ga.abs().max())
    a_ms, b_ms, p_ms = [], [], []
    for _ in range(args.rounds):                    # alternating
        a_ms.append(event_ms(arm_a, args.steps))
        b_ms.append(event_ms(arm_b, args.steps))
        p_ms.append(event_ms(probe, args.steps))
    a, b, p = statistics.median(a_ms), statistics.median(b_ms), statistics.median(p_ms)
    out = {"tool": "bench_store_gram", "model": args.model, "tasks": N, "r": r, "k": k, "parameters": P,
           "sum_rows": sum_rows, "units": int(plan.sizes.n_units), "rounds": args.rounds, "steps": args.steps,
           "device": torch.cuda.get_device_name(dev), "store_gram_read_bytes": int(read_bytes),
           "bytes_per_row_model": {"reconstruct_gram": 2 * r + 4 + 8 * N, "store_gram": 2 * r + 4},
           "gram_max_rel_diff_between_routes": rel,
           "reconstruct_gram_ms": _summary(a_ms), "store_gram_ms": _summary(b_ms), "probe_ms": _summary(p_ms),
           "reconstruct_gram_over_store_gram": round(a / b, 3),
           "store_gram_TBps": round(read_bytes / b / 1e9, 3), "probe_TBps": round(read_bytes / p / 1e9, 3),
           "store_gram_share_of_probe": round(p / b, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
