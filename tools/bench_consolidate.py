#!/usr/bin/env python3
"""What consolidating a STORE costs: svdq_plan_store_gram + svdq_plan_consolidate_eig + svdq_plan_rebase
(CompressPlan.consolidate: two reads of the stored basis, one write of the new one) against the only route there was
before it -- every task's model reconstructed (svdq_task_reconstruct for all N tasks, N fp32 models written) and
svdq_compress over the N outputs (read twice, a basis written) -- and against the read / write rate of the box.

Everything in ONE process on one GPU.  The store is the tool's own (tools/bench_store_gram.py's): for every visual
tensor of a CLIP model a random fp16 basis [rows, r = N] (k = N / 4 high columns), a random fp32 mean and random 4-bit
two-stage codes, adopted into one centred plan by svdq_plan_import.  Device events around --steps back-to-back calls,
--rounds rounds, the arms alternating inside a round, medians reported:

    materialise_ms   (a) reconstruct_tasks for all N tasks, then the compressor on the outputs
                     traffic model: rows * (2 r + 4) read + 4 N written + 4 N read twice + (2 r + 4) written
                     = 136 B/row at N = r = 8, 328 at 20
    consolidate_ms   (b) store_gram (with basis_gram), consolidate_eig, rebase: rows * (2 r + 4) read twice +
                     (2 r' + 4) written = 60 B/row at N = r = r' = 8, 132 at 20
    rebase_ms        the streaming pass of (b) alone
    probe_ms         svdq_hbm_probe mode 2 (read, write 5/8 of it) over as many bytes as the rebase pass reads

    python tools/bench_consolidate.py --model ViT-L-14 --tasks 8
    python tools/bench_consolidate.py --model ViT-L-14 --tasks 20

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
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from ctypes import c_void_p
    from svdq_amd import _native as nat, workloads
    from svdq_amd.pipeline import CompressPlan, _ptr, _stream_ptr, consolidate_views, keep_table, pack_small

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

    # (a) every task's reconstruction into one buffer, then the compressor over the N outputs
    offs, tot = [], 0
    for D in rows:
        offs.append(tot)
        tot += (D + 63) // 64 * 64
    outbuf = torch.empty(N * tot, dtype=torch.float32, device=dev)
    out_tab = torch.tensor([[outbuf.data_ptr() + 4 * (t * tot + offs[p]) for t in range(N)] for p in range(P)],
                           dtype=torch.int64).to(dev)
    cplan = CompressPlan(rows, N, center=True, fp16=True, low_bits=4, rtvq_stages=S, device=dev)
    ctab = out_tab.reshape(-1).contiguous()      # [P * N] parameter-major: the same pointers

    def arm_a():
        plan.reconstruct_tasks(list(range(N)), out_tab)
        cplan.run(ctab)

    # (b) the four launches, on buffers made once
    lib = nat.lib()
    dst = CompressPlan(rows, N, center=True, fp16=True, low_bits=4, rtvq_stages=S, device=dev, workspace=False)
    kt = keep_table(list(range(N)), P, N, N)
    kd = torch.from_numpy(kt).to(dev)
    lay = plan.consolidate_layout()
    tab = torch.zeros(int(lay.total_bytes), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.svdq_plan_store_gram_work_bytes(plan._h)), dtype=torch.uint8, device=dev)
    G = torch.empty((P, N, N), dtype=torch.float64, device=dev)
    M = torch.empty((P, 33, 33), dtype=torch.float64, device=dev)
    rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * P].view(torch.int64)

    def rebase():
        nat.check(lib.svdq_plan_rebase(plan._h, dst._h, _ptr(rows_dev), _ptr(plan.small), _ptr(plan.basis),
                                       _ptr(plan.mean), _ptr(tab), _ptr(dst.basis), _ptr(dst.mean), _stream_ptr()),
                  "svdq_plan_rebase")

    def arm_b():
        nat.check(lib.svdq_plan_store_gram(plan._h, _ptr(rows_dev), _ptr(plan.small), _ptr(plan.basis), _ptr(plan.mean),
                                           _ptr(work), _ptr(G), _ptr(M), _stream_ptr()), "svdq_plan_store_gram")
        nat.check(lib.svdq_plan_consolidate_eig(plan._h, dst._h, c_void_p(kt.ctypes.data), _ptr(kd), _ptr(rows_dev),
                                                _ptr(plan.small), _ptr(M), 0.0, _ptr(dst.small), _ptr(tab),
                                                _stream_ptr()), "svdq_plan_consolidate_eig")
        rebase()

    src = torch.empty(read_bytes, dtype=torch.uint8, device=dev).random_(0, 256)
    pdst = torch.empty(read_bytes, dtype=torch.uint8, device=dev)

    def probe():
        nat.check(lib.svdq_hbm_probe(2, c_void_p(src.data_ptr()), c_void_p(pdst.data_ptr()), read_bytes, _stream_ptr()),
                  "svdq_hbm_probe")

    def event_ms(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    arm_a()      # warm-up: code objects, work buffers, allocator
    arm_b()
    probe()
    torch.cuda.synchronize()
    fresh = cplan.fetch_small()
    t = consolidate_views(tab.cpu().numpy(), lay, P)
    big = int(np.argmax(rows))
    rn = int(t.r[big])
    sig_c = dst.fetch_small().sigma[big, :rn].astype(np.float64)
    sig_f = fresh.sigma[big, :rn].astype(np.float64)
    write_bytes = int(sum(D * (2 * int(t.r[p]) + 4) for p, D in enumerate(rows)))
    a_ms, b_ms, r_ms, p_ms = [], [], [], []
    for _ in range(args.rounds):                    # alternating
        a_ms.append(event_ms(arm_a, args.steps))
        b_ms.append(event_ms(arm_b, args.steps))
        r_ms.append(event_ms(rebase, args.steps))
        p_ms.append(event_ms(probe, args.steps))
    a, b, rb, p = (statistics.median(x) for x in (a_ms, b_ms, r_ms, p_ms))
    out = {"tool": "bench_consolidate", "model": args.model, "tasks": N, "r": r, "k": k, "parameters": P,
           "sum_rows": sum_rows, "units": int(plan.sizes.n_units), "rounds": args.rounds, "steps": args.steps,
           "device": torch.cuda.get_device_name(dev), "rebase_read_bytes": int(read_bytes),
           "rebase_write_bytes": write_bytes, "columns_kept_min_max": [int(t.r.min()), int(t.r.max())],
           "bytes_per_row_model": {"materialise": 2 * (2 * r + 4) + 12 * N, "consolidate": 3 * (2 * r + 4)},
           "sigma_max_rel_diff_between_routes_largest_tensor": float(np.abs(sig_c - sig_f).max() / sig_f[0]) if rn else 0.0,
           "materialise_ms": _summary(a_ms), "consolidate_ms": _summary(b_ms), "rebase_ms": _summary(r_ms),
           "probe_ms": _summary(p_ms), "materialise_over_consolidate": round(a / b, 3),
           "rebase_TBps": round((read_bytes + write_bytes) / rb / 1e9, 3),
           "probe_TBps": round((read_bytes + read_bytes * 5 // 8) / p / 1e9, 3),
           "rebase_share_of_probe": round(p / rb, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
