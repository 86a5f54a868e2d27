#!/usr/bin/env python3
"""Sign-elected (TIES, Yadav et al. 2023) merge of a stored artifact set, from the artifact directory and the base
checkpoint alone: trim every task's reconstruction to its largest magnitudes (--density), elect a sign per weight, average
the values that agree, add --scaling times the result to the base (storage.ties_merge_from_artifacts).  The task models
are never written: the values are formed pass by pass from the stored bases.  For stores of unmasked runs (masks are not
stored, reload.py:204-205).  Prints the thresholds and the kept counts as JSON lines."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="TIES merge of stored SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--base-model-path", required=True, help="Path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Path to save the merged model (default: not written)")
    ap.add_argument("--density", type=float, default=0.2,
                    help="Fraction of every task vector's entries the trim keeps, in (0, 1] (default 0.2)")
    ap.add_argument("--scaling", type=float, default=1.0, help="Factor on the merged task vector (default 1.0)")
    ap.add_argument("--merge-func", default="mean", choices=["mean", "sum"],
                    help="How the values that agree with the elected sign are combined (default mean)")
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
    from svdq_amd.storage import ties_merge_from_artifacts
    res = ties_merge_from_artifacts(args.artifact_dir, args.base_model_path, args.output_path, density=args.density,
                                    scaling=args.scaling, merge_func=args.merge_func, tasks=args.tasks, device=args.device)
    stats = res["stats"]
    print(json.dumps({"thresholds": stats["thresholds"]}))
    print(json.dumps({"kept": stats["kept"]}))
    print(json.dumps({"sign_conflict_rows": stats["sign_conflict_rows"], "empty_rows": stats["empty_rows"],
                      "rows": stats["rows"]}))
    where = f" -> {args.output_path}" if args.output_path else ""
    print(f"merged {len(res['merged_state_dict'])} entries{where}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
