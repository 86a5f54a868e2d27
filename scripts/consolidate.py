#!/usr/bin/env python3
"""Consolidate a stored artifact set: bases, rank, mean and coefficients re-derived from the artifacts alone
(storage.consolidate_artifacts) -- after add_task.py --extend-basis grew the store, to drop tasks from it (--tasks names
the ones to keep), or to take it to another energy threshold, maximum rank, code width or stage count.  The fine-tuned
checkpoints are not needed and no task model is materialised.  Without --output-dir the store is rewritten in place,
through a temporary directory beside it."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="Consolidate stored SVD-Hybrid artifacts without the fine-tuned checkpoints")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--output-dir", default=None, help="Directory for the consolidated store (default: in place)")
    ap.add_argument("--tasks", nargs="+", default=None, help="Tasks to keep (default: all)")
    ap.add_argument("--energy-threshold", type=float, default=None, help="svd_energy_threshold (default: as stored)")
    ap.add_argument("--max-rank", type=int, default=None, help="svd_max_rank (default: as stored)")
    ap.add_argument("--low-bits", type=int, default=None, help="svd_low_bits (default: as stored)")
    ap.add_argument("--stages", type=int, default=None, help="svd_rtvq_stages (default: as stored)")
    ap.add_argument("--min-sigma", type=float, default=0.0,
                    help="drop directions below this share of sigma_0 (default 0: the noise floor of the stored Gram alone)")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not os.path.exists(args.artifact_dir):
        ap.error(f"--artifact-dir: {args.artifact_dir} does not exist")
    from svdq_amd.storage import consolidate_artifacts
    res = consolidate_artifacts(args.artifact_dir, args.output_dir, tasks=args.tasks,
                                energy_threshold=args.energy_threshold, max_rank=args.max_rank, low_bits=args.low_bits,
                                rtvq_stages=args.stages, min_sigma=args.min_sigma, device=args.device)
    print("tasks: " + json.dumps(res["tasks"]))
    if res["dropped"]:
        print("dropped: " + json.dumps(res["dropped"]))
    before = sum(a for a, _ in res["columns"].values())
    after = sum(b for _, b in res["columns"].values())
    print(f"columns: {before} -> {after} over {len(res['columns'])} regions; dropped energy "
          f"{sum(res['dropped_energy'].values()):.3e}; {len(res['skipped'])} parameters skipped -> {res['output_dir']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
