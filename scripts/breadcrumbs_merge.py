#!/usr/bin/env python3
"""Model Breadcrumbs (Davari & Belilovsky 2023) merge of a stored artifact set, from the artifact directory and the base
checkpoint alone: per weight tensor and task keep the magnitudes between the small bulk and the few largest outliers
(--density of the entries, below the --gamma largest), optionally elect a sign per weight (--sign-election), add or
average what is left, add --scaling times the result to the base (storage.breadcrumbs_merge_from_artifacts).  With
--gamma 0 --sign-election --merge-func mean it is the per-tensor TIES trim.  The task models are never written: the values
are formed pass by pass from the stored bases.  For stores of unmasked runs (masks are not stored, reload.py:204-205).
Prints the kept counts per task and the row counters as JSON lines."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="Model Breadcrumbs merge of stored SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--base-model-path", required=True, help="Path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Path to save the merged model (default: not written)")
    ap.add_argument("--density", type=float, default=0.9,
                    help="Fraction of every tensor's entries the band keeps per task, in (0, 1] (default 0.9)")
    ap.add_argument("--gamma", type=float, default=0.01,
                    help="Fraction of every tensor's largest magnitudes cut per task, in [0, 1) (default 0.01)")
    ap.add_argument("--scaling", type=float, default=1.0, help="Factor on the merged task vector (default 1.0)")
    ap.add_argument("--sign-election", action="store_true",
                    help="Combine only the kept values whose sign agrees with the sign of their sum (default: all)")
    ap.add_argument("--merge-func", default="sum", choices=["mean", "sum"],
                    help="How the kept values are combined (default sum)")
    ap.add_argument("--tasks", nargs="+", default=None, help="Task names to merge (default: every stored task)")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    for what, path in (("--artifact-dir", args.artifact_dir), ("--base-model-path", args.base_model_path)):
        if not os.path.exists(path):
            ap.error(f"{what}: {path} does not exist")
    if not 0.0 < args.density <= 1.0:
        ap.error(f"--density: {args.density} is outside (0, 1]")
    if not 0.0 <= args.gamma < 1.0:
        ap.error(f"--gamma: {args.gamma} is outside [0, 1)")
    from svdq_amd.storage import breadcrumbs_merge_from_artifacts
    res = breadcrumbs_merge_from_artifacts(args.artifact_dir, args.base_model_path, args.output_path,
                                           density=args.density, gamma=args.gamma, scaling=args.scaling,
                                           sign_election=args.sign_election, merge_func=args.merge_func, tasks=args.tasks,
                                           device=args.device)
    stats = res["stats"]
    print(json.dumps({"kept_total": stats["kept_total"]}))
    print(json.dumps({"sign_conflict_rows": stats["sign_conflict_rows"], "empty_rows": stats["empty_rows"],
                      "rows": stats["rows"]}))
    where = f" -> {args.output_path}" if args.output_path else ""
    print(f"merged {len(res['merged_state_dict'])} entries{where}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
