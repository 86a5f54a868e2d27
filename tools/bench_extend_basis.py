#!/usr/bin/env python3
"""What growing the stored bases by the new tasks' out-of-span directions costs on the device: the launches of
svdq_plan_residual_gram (the streaming residual-Gram pass and the per-parameter eigen stage, one entry point) and of
svdq_plan_extend_basis (the streaming write pass), beside svdq_plan_project on the same plan, each against the read rate.

The method is tools/bench_project_tasks.py's: ONE process on one GPU, the store made by the fused run of
svdq_amd.workloads' synthetic task vectors and turned into plain dictionaries, --new further task vectors as the new
tasks; device events over --steps back-to-back calls, --reps rounds alternating with torch's read-only sum of a 4 GiB
buffer (the read ceiling of tools/hbm_ceiling.py).

  bytes a pass must move, per row of an entry: e r + 4 (basis and mean) + 4 per new task; the write pass also writes
  e (k + m).  The eigen stage moves next to nothing (one fp64 [8][8] partial per work unit).

    python tools/bench_extend_basis.py --model ViT-L-14 --tasks 8 --new 1
    python tools/bench_extend_basis.py --model ViT-B-16 --tasks 8 --new 8

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _to(obj, device):
    if isinstance(obj, torch.Tensor):
        return obj.detach().to(device).clone()
    if isinstance(obj, dict):
        return {k: _to(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and not isinstance(obj, torch.Size):
        return type(obj)(_to(v, device) for v in obj)
    return obj


def _summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "runs": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8, help="tasks of the stored set")
    ap.add_argument("--new", type=int, default=1, help="new tasks (1..8)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd
    from svdq_amd import workloads
    from svdq_amd.driver import adopt_bases

    N, M = args.tasks, args.new
    shapes = workloads.vit_visual_shapes(args.model)
    names = sorted(shapes)
    rows = [workloads.numel(shapes[n]) for n in names]
    old = [f"task{t:02d}" for t in range(N)]
    new = [f"new{t:02d}" for t in range(M)]
    _, views = workloads.synth_task_buffers(rows, N + M, seed=0, device=dev)
    tv = {t: {n: views[p][j].view(shapes[n]) for p, n in enumerate(names)} for j, t in enumerate(old + new)}
    cfg = svdq_amd.SVDHybridConfig(tasks=old, svd_energy_threshold=0.9, svd_max_rank=64, svd_low_bits=4, svd_rtvq_stages=2)
    bases, comp = svdq_amd.run_basis_and_compress({t: tv[t] for t in old}, None, cfg, dev)
    plain_b = {n: {r: (_to(dict(b.items()), dev) if b is not None else None) for r, b in bases[n].items()} for n in names}
    del bases, comp
    batches, declined = adopt_bases(plain_b, cfg, M, device=dev)
    assert len(batches) == 1 and not declined, (len(batches), declined)
    batch = batches[0]
    plan = batch.plan
    tab, keep = [0] * (plan.P * plan.N), []
    for i, (name, _) in enumerate(batch.entries):
        for j, t in enumerate(new):
            v = tv[t][name].reshape(-1)
            keep.append(v)
            tab[i * plan.N + j] = v.data_ptr()
    table = torch.tensor(tab, dtype=torch.int64).to(dev)
    sm = plan.project_tasks(table)
    ext = plan.residual_gram(table, M)
    es = 2 if plan.fp16 else 4
    udt = torch.float16 if plan.fp16 else torch.float32
    outs = [torch.empty((int(sm.rows[i]), int(sm.k[i]) + int(ext.m[i])), dtype=udt, device=dev) if ext.m[i] > 0 else None
            for i in range(plan.P)]
    read = sum(int(sm.rows[i]) * (es * int(sm.r[i]) + 4 + 4 * M) for i in range(plan.P))
    wrote = sum(int(sm.rows[i]) * es * (int(sm.k[i]) + int(ext.m[i])) for i in range(plan.P) if ext.m[i] > 0)
    x = torch.randn(1 << 30, device=dev)

    def event_ms(fn, steps):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    runs = {"project": [], "residual_gram": [], "extend_basis": [], "read": []}
    for _ in range(args.reps):             # alternating
        runs["project"].append(event_ms(lambda: plan.project_tasks(table, fetch=False), args.steps))
        runs["residual_gram"].append(event_ms(lambda: plan.residual_gram(table, M, fetch=False), args.steps))
        runs["extend_basis"].append(event_ms(lambda: plan.extend_basis(table, M, outs), args.steps))
        runs["read"].append(event_ms(lambda: x.sum(), args.steps))
    med = {k: statistics.median(v) for k, v in runs.items()}
    ceiling = 4 * x.numel() / med["read"] / 1e9
    out = {"tool": "bench_extend_basis", "model": args.model, "stored_tasks": N, "new_tasks": M, "parameters": len(names),
           "sum_rows": int(sum(rows)), "reps": args.reps, "steps": args.steps, "device": torch.cuda.get_device_name(dev),
           "plan_tasks": plan.N, "units": int(plan.sizes.n_units), "new_columns": int(ext.m.sum()),
           "read_4GiB_ms": _summary(runs["read"]), "read_ceiling_TBps": round(ceiling, 3)}
    for key, must in (("project", read), ("residual_gram", read), ("extend_basis", read + wrote)):
        tbps = must / med[key] / 1e9
        out[key] = {"ms": _summary(runs[key]), "bytes_must_move": must, "TBps": round(tbps, 3),
                    "share_of_read_ceiling": round(tbps / ceiling, 4)}
    out["residual_gram"]["launches"] = "streaming residual-Gram pass + per-parameter eigen stage"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
