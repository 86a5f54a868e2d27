"""Regenerates the figures behind helpers.BASIS_ROWS_G0 / BASIS_ROWS_G / BASIS_ROWS_C ("Basis and
mean, row by row"): the reference chain on the CPU (LAPACK fp32 SVD, .half(), fp32 GEMVs) over every shape of
tests/test_hip_basis_rows.py with the fitted terms switched off, and per storage type what the chain needs.  No GPU.

    python tools/fit_basis_rows.py [--threads T] [--large-only | --no-large] [--jsonl FILE]

LAPACK's blocking depends on the thread count and the figures of the 4 M-row shapes move with it (the others do not):
run it at the thread counts of interest; the committed constants are twice the largest need seen."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--jsonl", default=None, help="also write one line per chain")
    a = ap.parse_args()
    import numpy as np
    import torch
    if a.threads:
        torch.set_num_threads(a.threads)
    import helpers as H
    from oracle import svd_hybrid_oracle as orc

    cases = []
    if not a.large_only:
        cases += [(D, N, fp16, center, ur) for N in H.BASIS_ROWS_N for ur in (0, 1024) for D in H.basis_rows_sizes(N)
                  for center in (True, False) for fp16 in (True, False)]
    if not a.no_large:
        cases += [(D, N, fp16, center, 0) for D, N, fp16, center in H.BASIS_ROWS_LARGE]
    log = open(a.jsonl, "w") if a.jsonl else None
    need = {}      # (fp16, size class) -> largest figures
    last, deltas = None, None
    for D, N, fp16, center, ur in cases:
        if last != (D, N, ur):
            deltas, last = H.basis_rows_inputs(orc, D, N, ur), (D, N, ur)
        out = H.reference_chain(orc, deltas, center, fp16)
        s = H.basis_rows_ratios(deltas, *out, fp16, center, g0=0.0, g=0.0, c=0.0)
        cls = "D < 64" if D < H.BASIS_ROWS_SMALL else ("D >= 64" if D < 10 ** 6 else "D = 4 M")
        n = need.setdefault((fp16, cls), dict(a0=0.0, g_flat=0.0, g_sqrtD=0.0, b=0.0, c_err=0.0, c_need=0.0, chains=0))
        n["chains"] += 1
        n["a0"] = max(n["a0"], s["a0"])
        n["g_flat"] = max(n["g_flat"], s["a_need"])
        n["g_sqrtD"] = max(n["g_sqrtD"], s["a_need"] / np.sqrt(D))
        n["b"] = max(n["b"], s["b"])
        n["c_err"] = max(n["c_err"], s["c_err"])
        n["c_need"] = max(n["c_need"], s["c_need"])
        if log:
            log.write(json.dumps(dict(D=D, N=N, fp16=fp16, center=center, unit_rows=ur, a0=s["a0"], g_need=s["a_need"],
                                      b=s["b"], c_err=s["c_err"], c_need=s["c_need"])) + "\n")
            log.flush()
    print(f"threads {torch.get_num_threads()}")
    for (fp16, cls), n in sorted(need.items(), key=lambda kv: (not kv[0][0], kv[0][1])):
        print(f"{'fp16' if fp16 else 'fp32'} basis, {cls:8s} ({n['chains']:4d} chains): (a) error/bound without g "
              f"{n['a0']:.3g}, g needed {n['g_flat']:.4g} = {n['g_sqrtD']:.4g} sqrt(D); (b) {n['b']:.3f}; "
              f"(c) |U^T U - I| {n['c_err']:.3g}, c needed {n['c_need']:.4g}")


if __name__ == "__main__":
    main()
