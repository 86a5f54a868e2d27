#!/usr/bin/env python3
"""What the EMR merge of a store costs, in time and in peak memory: the fused route (merge.emr_merge_parameters: one pass
over the basis, no task model written; merge.emr_task_state_dict: one launch per task model) against the materialised
route built only from pieces the package had before -- ``reconstruct_task_vectors`` for all tasks, the same definition
in torch (sum, sign, agreeing maximum, compares, two fp64 sums per task) and ``numpy.packbits`` on the host; its task
model is ``base + lambda * where(mask, tau, 0)`` in torch.  The materialised route is the yardstick.

Everything in ONE process on one GPU: the bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for
every visual tensor of a CLIP model; ViT-L-14 x 8 by default) goes through ``run_basis_and_compress`` once, the task
vectors are dropped, the dictionaries stay resident.  Before any timing the routes are compared: torch's reduction may add
the tasks in another order, so a row's elected sign may differ where the sum is within T 2^-23 sum|v| of zero; the
differing mask bits are counted and reported (more than 1 in 1000 stops the tool), and the rescalers must agree within
1e-3 relative.  Then, alternating, a host clock around calls that end in a device synchronise (the host's table building
is part of what a caller pays), --reps rounds of --calls calls each; ``torch.cuda.max_memory_allocated`` over the value
just before the call is recorded for one call of each route.  A read-rate probe of the box (svdq_hbm_probe, mode 0, 1 GiB)
stands beside the figures.

    python tools/bench_emr_merge.py --out profiles/emr_merge_vitl8.json
    python tools/bench_emr_merge.py --tasks 20 --out profiles/emr_merge_vitl20.json

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_emr_merge.py --calls 1
--reps 1 --with-parents``: --with-parents adds one consensus merge with masks of the same store to the process, so that
k_tall_consensus (the same reads, the same two sweeps, the same stream words, one fp32 tensor written) stands in the
same trace.  Prints one JSON line (and writes it to --out).
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


def materialised(sq, comp, bases, shapes, cfg, names, tasks):
    """The definition on the T reconstructed task vectors.  Returns (tau [D], packed uint8 [T, bytes], A, B float64 [T])."""
    import numpy as np
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    M = torch.stack([torch.cat([recon[t][n].reshape(-1) for n in names]) for t in tasks])      # [T, D]
    del recon
    S = M.sum(dim=0)
    gamma = torch.sign(S)
    bits = (M * gamma.unsqueeze(0)) > 0
    eps = torch.where(bits, M.abs(), torch.zeros_like(M)).amax(dim=0)
    tau = eps * gamma
    A = M.abs().sum(dim=1, dtype=torch.float64)
    B = torch.where(bits, eps.unsqueeze(0), torch.zeros_like(M)).sum(dim=1, dtype=torch.float64)
    packed = np.packbits(bits.cpu().numpy(), axis=1)
    return tau, packed, A, B


def probe_read_rate(sq, dev):
    """TB/s of a plain streaming read of 1 GiB on this box (svdq_hbm_probe mode 0), the median of 5."""
    from svdq_amd.pipeline import _ptr, _stream_ptr
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev).zero_()
    dst = torch.empty(n, dtype=torch.uint8, device=dev)
    lib = sq._native.lib()
    rates = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sq._native.check(lib.svdq_hbm_probe(0, _ptr(src), _ptr(dst), n, _stream_ptr()), "svdq_hbm_probe")
        torch.cuda.synchronize()
        if i:
            rates.append(n / (time.perf_counter() - t0) / 1e12)
    return round(statistics.median(rates), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed round and route")
    ap.add_argument("--with-parents", action="store_true",
                    help="also run one consensus merge with masks (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd as sq
    from svdq_amd import workloads
    N = args.tasks
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
    print("compressed", file=sys.stderr, flush=True)
    shapes = {n: torch.Size([r]) for n, r in zip(names, rows)}
    D = sum(rows)
    r_mean = sum(int(bases[n]["masked"]["k"] + bases[n]["masked"]["U_low"].shape[1]) * r for n, r in zip(names, rows)) / D
    read_rate = probe_read_rate(sq, dev)
    base = {n: torch.randn(r, device=dev) for n, r in zip(names, rows)}

    def sync(x):
        torch.cuda.synchronize()
        return x

    def run_elect():
        return sync(sq.emr_merge_parameters(comp, bases, shapes, cfg, device="cuda", return_stats=True))

    def run_materialised():
        return sync(materialised(sq, comp, bases, shapes, cfg, names, tasks))

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        res = fn()
        return res, torch.cuda.max_memory_allocated() - before

    (unified, masks, rescalers, stats), peak_elect = peak_of(run_elect)
    (tau, packed, A, B), peak_mat = peak_of(run_materialised)
    # ---- the routes against each other
    fused_bits = torch.stack([masks[t] for t in tasks])
    diff = fused_bits ^ torch.from_numpy(packed).to(dev)
    differing = int(sum(int((diff >> i & 1).sum()) for i in range(8)))
    fused_tau = torch.cat([unified[n].reshape(-1) for n in names])
    tau_rows_differing = int((fused_tau != tau).sum())
    lam_mat = (A / B).tolist()
    lam_worst = max(abs(rescalers[t] - lam_mat[g]) / lam_mat[g] for g, t in enumerate(tasks))
    if differing > 1e-3 * N * D or lam_worst > 1e-3:
        raise SystemExit(f"the routes disagree: {differing} of {N * D} mask bits differ, rescalers by {lam_worst}")
    del diff, fused_bits, packed
    t_apply = tasks[N // 2]
    lam = float(torch.tensor(rescalers[t_apply], dtype=torch.float32))
    g_apply = tasks.index(t_apply)

    def run_apply():
        return sync(sq.emr_task_state_dict(unified, masks, rescalers, t_apply, base_state_dict=base, device="cuda"))

    # the materialised apply keeps an unpacked bool mask of the task, as a caller of the old route would
    import numpy as np
    mask_bool = torch.from_numpy(np.unpackbits(masks[t_apply].cpu().numpy())[:D].astype(bool)).to(dev)
    base_flat = torch.cat([base[n] for n in names])

    def run_apply_materialised():
        return sync(base_flat + lam * torch.where(mask_bool, tau, torch.zeros_like(tau)))

    out_f, peak_apply = peak_of(run_apply)
    out_m, peak_apply_mat = peak_of(run_apply_materialised)
    apply_rows_differing = int((torch.cat([out_f[n].reshape(-1) for n in names]) != out_m).sum())
    del out_f, out_m
    torch.cuda.empty_cache()
    print("routes compared", file=sys.stderr, flush=True)
    if args.with_parents:
        sync(sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=0.4, k=2, return_masks=True, device="cuda"))

    def wall_ms(fn):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    routes = {"fused_elect_ms": run_elect, "materialised_elect_ms": run_materialised, "fused_apply_ms": run_apply,
              "materialised_apply_ms": run_apply_materialised}
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating; the comparison above was the warm-up of all four
        for key, fn in routes.items():
            times[key].append(wall_ms(fn))
        print("round timed", file=sys.stderr, flush=True)
    es = 2 if cfg.svd_fp16 else 4
    n_units = sum(b.plan.sizes.n_units for b in {id(bases[n]["masked"]._batch[0]): bases[n]["masked"]._batch[0]
                                                 for n in names}.values())
    out = {"tool": "bench_emr_merge", "model": args.model, "tasks": N, "parameters": len(names), "sum_rows": D,
           "mean_rank": round(r_mean, 3), "work_units": n_units, "device": torch.cuda.get_device_name(dev),
           "read_rate_probe_TBps": read_rate, "reps": args.reps, "calls_per_round": args.calls,
           "mask_bits_differing_from_materialised": differing, "mask_bits": N * D,
           "tau_rows_differing_from_materialised": tau_rows_differing,
           "apply_rows_differing_from_materialised": apply_rows_differing,
           "rescaler_worst_relative_difference": lam_worst,
           "rescalers": {t: round(rescalers[t], 6) for t in tasks},
           "density": {t: round(stats["active"][t] / D, 4) for t in tasks}, "applied_task": t_apply,
           "applied_task_index": g_apply, "model_bytes": 4 * D,
           "peak_rise_bytes": {"fused_elect": int(peak_elect), "materialised_elect": int(peak_mat),
                               "fused_apply": int(peak_apply), "materialised_apply": int(peak_apply_mat)},
           "peak_rise_models": {"fused_elect": round(peak_elect / (4 * D), 3),
                                "materialised_elect": round(peak_mat / (4 * D), 3),
                                "fused_apply": round(peak_apply / (4 * D), 3),
                                "materialised_apply": round(peak_apply_mat / (4 * D), 3)},
           # elect: reads basis + mean, writes tau_uni and T bits per row; apply: reads tau_uni, base and 1 bit, writes fp32
           "bytes_per_row_model": {"elect_read": round(es * r_mean + 4, 3), "elect_written": round(4 + N / 8, 3),
                                   "apply_read": 8.125, "apply_written": 4},
           "bytes_moved_elect": int(D * (es * r_mean + 4) + D * (4 + N / 8)), "bytes_moved_apply": int(D * 12.125)}
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    out["materialised_over_fused_elect"] = round(out["materialised_elect_ms"]["median"] / out["fused_elect_ms"]["median"], 3)
    out["materialised_over_fused_apply"] = round(out["materialised_apply_ms"]["median"] / out["fused_apply_ms"]["median"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
