#!/usr/bin/env python3
"""What TALL masks and a consensus merge of a store cost, in time and in peak memory: the fused route
(merge.consensus_merge_parameters / merge.tall_masks_from_store: one pass over the basis, no task model written) as merge +
masks, merge only and masks only, against the materialised route built only from pieces the package had before --
``reconstruct_task_vectors`` for all tasks, ``torch.stack(...).sum``, T compares, the count and the packing.  The
materialised route is the yardstick.  Its packing is done where it is faster: both ways (eight shifted adds on the device;
``numpy.packbits`` on the host after the copy) are timed once and the JSON line says which one the timed route uses.

Everything in ONE process on one GPU: the bench.py workload (svdq_amd.workloads' synthetic task vectors, from a seed, for
every visual tensor of a CLIP model; ViT-L-14 x 8 by default) goes through ``run_basis_and_compress`` once, the task
vectors are dropped, the dictionaries stay resident.  Before any timing the routes are compared: torch's reduction may add
in another order, so the sums at k = 0 must agree within T 2^-23 sum|v| per row, and the mask bits may differ only where a
comparison is that close to a tie (the differing bits are counted and reported; more than 1 in 1000 stops the tool).
Then, alternating, a host clock around calls that end in a device synchronise (the host's table building is part of what
a caller pays), --reps rounds of --calls calls each; ``torch.cuda.max_memory_allocated`` over the value just before the
call is recorded for one call of each route.

    python tools/bench_tall_consensus.py --out profiles/tall_consensus_vitl8.json
    python tools/bench_tall_consensus.py --tasks 20 --out profiles/tall_consensus_vitl20.json

Kernel time: a run of its own under ``rocprofv3 --kernel-trace --stats -- python tools/bench_tall_consensus.py --calls 1
--reps 1 --with-parents``: --with-parents adds one TIES merge and one DARE merge at drop rate 0 of the same store to the
process, so that k_ties_merge (the same two-sweep structure) and k_dare_merge (the one-sweep floor) stand in the same
trace.  Prints one JSON line (and writes it to --out).
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


def pack_device(bits):
    """uint8 [T, ceil(D / 8)] from bool [T, D] in numpy.packbits order."""
    T, D = bits.shape
    pad = (-D) % 8
    if pad:
        bits = torch.nn.functional.pad(bits, (0, pad))
    b = bits.view(T, -1, 8).to(torch.uint8)
    out = torch.zeros(b.shape[:2], dtype=torch.uint8, device=bits.device)
    for i in range(8):
        out += b[:, :, i] << (7 - i)
    return out


def pack_host(bits):
    import numpy as np
    return np.packbits(bits.cpu().numpy(), axis=1)


def materialised(sq, comp, bases, shapes, cfg, names, tasks, lam, k, pack):
    """Sum, compares, count and packing on the T reconstructed task vectors.  Returns (merged [D], packed, count [D])."""
    recon = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, device="cuda")
    M = torch.stack([torch.cat([recon[t][n].reshape(-1) for n in names]) for t in tasks])      # [T, D]
    del recon
    S = M.sum(dim=0)
    bits = M.abs() > lam * (S.unsqueeze(0) - M).abs()
    count = bits.sum(dim=0)
    merged = torch.where(count >= k, S, torch.zeros_like(S))
    return merged, pack(bits), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--tasks", type=int, default=8)
    ap.add_argument("--tall-lambda", type=float, default=0.4)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed round and route")
    ap.add_argument("--with-parents", action="store_true",
                    help="also run one TIES merge and one DARE merge at drop rate 0 (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import svdq_amd as sq
    from svdq_amd import workloads
    N, lam, k = args.tasks, args.tall_lambda, args.k
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

    def sync(x):
        torch.cuda.synchronize()
        return x

    def run_both(kk=k):
        return sync(sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=lam, k=kk, return_masks=True,
                                                  device="cuda", return_stats=True))

    def run_merge():
        return sync(sq.consensus_merge_parameters(comp, bases, shapes, cfg, tall_lambda=lam, k=k, device="cuda",
                                                  return_stats=True))

    def run_masks():
        return sync(sq.tall_masks_from_store(comp, bases, shapes, cfg, tall_lambda=lam, device="cuda", return_stats=True))

    def timed_once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, (time.perf_counter() - t0) * 1e3

    # ---- which packing the yardstick uses
    probe = torch.rand((N, D), device=dev) < 0.5
    pack_device(probe[:, :1024])
    pd, dev_ms = timed_once(lambda: pack_device(probe))
    ph, host_ms = timed_once(lambda: pack_host(probe))
    if not (pd.cpu().numpy() == ph).all():
        raise SystemExit("the two packings disagree")
    del probe, pd, ph
    pack = pack_device if dev_ms <= host_ms else pack_host

    def run_materialised(kk=k):
        return sync(materialised(sq, comp, bases, shapes, cfg, names, tasks, lam, kk, pack))

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        res = fn()
        return res, torch.cuda.max_memory_allocated() - before

    (_, masks, stats), peak_both = peak_of(run_both)
    _, peak_merge = peak_of(run_merge)
    _, peak_masks = peak_of(run_masks)
    (_, packed, count), peak_mat = peak_of(run_materialised)
    # ---- the routes against each other
    fused_bits = torch.stack([masks[t] for t in tasks])
    packed = packed if isinstance(packed, torch.Tensor) else torch.from_numpy(packed).to(dev)
    diff = fused_bits ^ packed
    differing = int(sum(int((diff >> i & 1).sum()) for i in range(8)))
    agreement_mat = torch.bincount(count, minlength=N + 1).tolist()
    del masks, packed, count, diff, fused_bits
    fused0 = run_both(0)[0]
    mat0 = run_materialised(0)[0]
    bound = torch.zeros(D, device=dev, dtype=torch.float64)
    for t in tasks:
        rec = sq.reconstruct_task_vectors(comp, bases, {}, shapes, cfg, tasks=[t], device="cuda")[t]
        bound += torch.cat([rec[n].reshape(-1) for n in names]).abs().double()
        del rec
    bound *= N * 2.0 ** -23
    err = (torch.cat([fused0[n].reshape(-1) for n in names]).double() - mat0.double()).abs()
    within = bool((err <= bound).all())
    worst = float(err.max())
    if not within or differing > 1e-3 * N * D:
        raise SystemExit(f"the routes disagree: sums at k = 0 within the bound {within} (worst {worst}), {differing} of "
                         f"{N * D} mask bits differ")
    del fused0, mat0, bound, err
    torch.cuda.empty_cache()
    print("routes compared", file=sys.stderr, flush=True)
    if args.with_parents:
        sync(sq.ties_merge_parameters(comp, bases, shapes, cfg, density=0.2, device="cuda"))
        sync(sq.dare_merge_parameters(comp, bases, shapes, cfg, drop_rate=0.0, device="cuda"))

    def wall_ms(fn):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    routes = {"fused_merge_and_masks_ms": run_both, "fused_merge_only_ms": run_merge, "fused_masks_only_ms": run_masks,
              "materialised_ms": run_materialised}
    times = {key: [] for key in routes}
    for _ in range(args.reps):          # alternating; the comparison above was the warm-up of all four
        for key, fn in routes.items():
            times[key].append(wall_ms(fn))
        print("round timed", file=sys.stderr, flush=True)
    es = 2 if cfg.svd_fp16 else 4
    density = {t: round(stats["active"][t] / D, 4) for t in tasks}
    out = {"tool": "bench_tall_consensus", "model": args.model, "tasks": N, "parameters": len(names), "sum_rows": D,
           "mean_rank": round(r_mean, 3), "tall_lambda": lam, "k": k, "device": torch.cuda.get_device_name(dev),
           "reps": args.reps, "calls_per_round": args.calls, "k0_sums_within_bound": within,
           "k0_worst_abs_difference": worst, "mask_bits_differing_from_materialised": differing, "mask_bits": N * D,
           "density": density, "agreement": stats["agreement"], "agreement_materialised": agreement_mat,
           "materialised_packing": "device" if pack is pack_device else "host",
           "packing_probe_ms": {"device": round(dev_ms, 3), "host": round(host_ms, 3)}, "model_bytes": 4 * D,
           "peak_rise_bytes": {"fused_merge_and_masks": int(peak_both), "fused_merge_only": int(peak_merge),
                               "fused_masks_only": int(peak_masks), "materialised": int(peak_mat)},
           "peak_rise_models": {"fused_merge_and_masks": round(peak_both / (4 * D), 3),
                                "fused_merge_only": round(peak_merge / (4 * D), 3),
                                "fused_masks_only": round(peak_masks / (4 * D), 3),
                                "materialised": round(peak_mat / (4 * D), 3)},
           # one pass: reads basis + mean, writes the output and T bits per row
           "bytes_per_row_model": {"read": round(es * r_mean + 4, 3), "written": round(4 + N / 8, 3)},
           "bytes_moved_fused": int(D * (es * r_mean + 4) + D * (4 + N / 8))}
    for key in routes:
        out[key] = {"median": round(statistics.median(times[key]), 3), "rounds": [round(x, 3) for x in times[key]]}
    out["materialised_over_fused"] = round(out["materialised_ms"]["median"] / out["fused_merge_and_masks_ms"]["median"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
