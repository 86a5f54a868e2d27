#!/usr/bin/env python3
"""What the reconstruction diagnostics cost with and without materialised task vectors.

Everything in ONE process on one GPU: a base model and N fine-tuned models (base + svdq_amd.workloads' synthetic task
vectors, from a seed, for every visual tensor of a CLIP model, stored as --dtype) are compressed once straight from the
checkpoints; the artifacts stay resident.  Before any timing the from-base result is compared bit for bit with the
result on the materialised fp32 deltas (the tool fails otherwise).  Then, alternating, device events around --seconds
worth of back-to-back calls each, --reps rounds:
    (a) diag_resident_ms     svdq_diagnostics on N resident fp32 deltas
    (b) ingest_plus_diag_ms  svdq_ingest (fp32 fine-tuned and base in, N fp32 deltas out) + (a): the materialising route
    (c) diag_from_base_ms    svdq_diagnostics_from_base on the fine-tuned and base tensors as stored (--dtype)
bytes per row, from shapes and the ranks in the small buffer: (a) 4 N + e r, (b) 4 (2 N + 1) more, (c) s (N + 1) + e r
with s the checkpoint element size and e the basis element size.

    python tools/bench_diag_from_base.py --tasks 8
    python tools/bench_diag_from_base.py --tasks 20 --dtype bfloat16

``--masks union``: the same three on MASKED parameters (bench.py --masks union's masks: per-task rand > 0.7 from seed 77,
combined by union; ViT-B-16 x 8 unless told otherwise; fp32 only): svdq_diagnostics_masked, svdq_ingest +
svdq_diagnostics_masked, svdq_diagnostics_masked_from_base.

    python tools/bench_diag_from_base.py --masks union

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_diag_from_base.py ...``.
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
    ap.add_argument("--model", default=None, help="default: ViT-L-14, with --masks ViT-B-16")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--dtype", choices=("float32", "float16", "bfloat16"), default="float32",
                    help="element type the checkpoints are stored in (the masked form reads float32 only)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of each timed window")
    ap.add_argument("--masks", choices=("none", "union"), default="none")
    args = ap.parse_args()
    masked = args.masks != "none"
    if masked and args.dtype != "float32":
        ap.error("--masks union reads float32 checkpoints only")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd  # noqa: F401
    from svdq_amd import _native as nat, workloads
    from svdq_amd.mask_loader import MaskSet
    from svdq_amd.pipeline import CompressPlan
    model = args.model or ("ViT-B-16" if masked else "ViT-L-14")
    dtype = getattr(torch, args.dtype)
    N = args.tasks
    shapes = workloads.vit_visual_shapes(model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    P = len(rows)
    offs, tot = [], 0
    for r in rows:      # synth_task_buffers' layout: 64-element aligned slices of one buffer per task
        offs.append(tot)
        tot += (r + 63) // 64 * 64

    def views(buf):
        return [buf[o:o + r] for o, r in zip(offs, rows)]

    def table(tensors):
        return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(dev)

    task_bufs, _ = workloads.synth_task_buffers(rows, N, seed=0, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    base_buf = torch.randn(tot, generator=g, device=dev).to(dtype)
    ft_bufs = [(base_buf.float() + tb[:tot]).to(dtype) for tb in task_bufs]
    del task_bufs
    # the materialising route works on fp32: its inputs (the checkpoints widened once, outside the timing) and its deltas
    base32 = base_buf if dtype is torch.float32 else base_buf.float()
    ft32 = ft_bufs if dtype is torch.float32 else [f.float() for f in ft_bufs]
    delta_bufs = [torch.empty(tot, dtype=torch.float32, device=dev) for _ in range(N)]
    pm = lambda per_task: [v[p] for p in range(P) for v in per_task]      # [P * N], parameter-major
    ft_tab, base_tab = table(pm([views(f) for f in ft_bufs])), table(views(base_buf))
    ft32_tab, base32_tab = table(pm([views(f) for f in ft32])), table(views(base32))
    delta_tab = table(pm([views(d) for d in delta_bufs]))

    kw = dict(energy_threshold=0.9, max_rank=64, center=True, fp16=True, low_bits=4, rtvq_stages=2, device=dev)
    plan = CompressPlan(rows, N, input_dtype=dtype, **kw)            # reads the checkpoints as stored
    p32 = plan if dtype is torch.float32 else CompressPlan(rows, N, **kw)   # reads the fp32 deltas, same artifacts
    lib, vp = nat.lib(), ctypes.c_void_p

    def ingest():
        nat.check(lib.svdq_ingest(p32._h, vp(base32_tab.data_ptr()), vp(ft32_tab.data_ptr()), vp(delta_tab.data_ptr()),
                                  vp(0), vp(torch.cuda.current_stream().cuda_stream)), "svdq_ingest")

    ingest()
    mtab = us = rows_dev = None
    if masked:
        gm = torch.Generator(device=dev).manual_seed(77)
        union = torch.zeros(tot, dtype=torch.bool, device=dev)
        for _ in range(N):
            union |= torch.rand(tot, device=dev, generator=gm) > 0.7
        ms = MaskSet(rows, dev)
        rows_dev, _ = ms.count_scan(views(union))
        mtab = table(ms._s["mb"])
        us = ms.unit_starts(plan, rows_dev, entry_map=[(q, False) for q in range(P)])
        plan.run_masked_from_base(ft_tab, base_tab, mtab, us, rows_dev)
    else:
        plan.run_from_base(ft_tab, base_tab)
        if p32 is not plan:
            p32.run(delta_tab)
            p32.fetch_small()
    sm = plan.fetch_small()
    if p32 is not plan and not torch.equal(plan.small, p32.small):
        raise SystemExit("the half plan and the fp32 plan disagree on the small artifacts")

    if masked:
        run_a = lambda: plan.diagnostics_masked(delta_tab, mtab, us, rows_dev)
        run_c = lambda: plan.diagnostics_masked_from_base(ft_tab, base_tab, mtab, us, rows_dev)
    else:
        run_a = lambda: p32.diagnostics(delta_tab)
        run_c = lambda: plan.diagnostics_from_base(ft_tab, base_tab)

    def run_b():
        ingest()
        return run_a()

    a, c = run_a(), run_c()
    torch.cuda.synchronize()
    same = torch.equal(a.view(torch.int64), c.view(torch.int64))
    if not same:
        raise SystemExit("diagnostics from base and diagnostics on the materialised deltas differ in bits")
    finite_share = float(torch.isfinite(a).all(dim=-1).float().mean())

    def event_ms(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    routes = {"diag_resident_ms": run_a, "ingest_plus_diag_ms": run_b, "diag_from_base_ms": run_c}
    steps = {}
    for key, fn in routes.items():      # warm-up, and how many calls fill the window
        event_ms(fn, 3)
        steps[key] = max(3, math.ceil(args.seconds * 1e3 / event_ms(fn, 5)))
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating
        for key, fn in routes.items():
            times[key].append(event_ms(fn, steps[key]))
    med = {key: statistics.median(v) for key, v in times.items()}
    s, e = base_buf.element_size(), 2
    src = rows if masked else [int(x) for x in sm.rows]      # rows the task tensors are read over (walk: every source row)
    ubytes = sum(int(sm.rows[p]) * e * int(sm.r[p]) for p in range(P))
    bytes_a = sum(src) * (4 * N + (1 if masked else 0)) + ubytes
    bytes_c = sum(src) * (s * (N + 1) + (1 if masked else 0)) + ubytes
    bytes_ingest = sum(rows) * 4 * (2 * N + 1)
    out = {"tool": "bench_diag_from_base", "model": model, "tasks": N, "dtype": args.dtype, "masks": args.masks,
           "parameters": P, "units": int(plan.sizes.n_units), "sum_rows": int(sum(rows)),
           "selected_rows": int(sum(int(x) for x in sm.rows)), "reps": args.reps, "window_s": args.seconds, "steps": steps,
           "device": torch.cuda.get_device_name(dev), "same_bits": bool(same), "finite_share": round(finite_share, 4),
           "bytes_diag_resident": bytes_a, "bytes_ingest": bytes_ingest, "bytes_diag_from_base": bytes_c}
    for key in routes:
        out[key] = {"median": round(med[key], 4), "rounds": [round(x, 4) for x in times[key]]}
    out["from_base_over_resident"] = round(med["diag_from_base_ms"] / med["diag_resident_ms"], 4)
    out["ingest_plus_diag_over_from_base"] = round(med["ingest_plus_diag_ms"] / med["diag_from_base_ms"], 4)
    out["resident_TBps"] = round(bytes_a / med["diag_resident_ms"] / 1e9, 3)
    out["from_base_TBps"] = round(bytes_c / med["diag_from_base_ms"] / 1e9, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
