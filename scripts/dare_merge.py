#!/usr/bin/env python3
"""Drop-and-rescale (DARE, Yu et al. 2024) merge of a stored artifact set, from the artifact directory and the base
checkpoint alone: thin every task's reconstruction by a random mask (--drop-rate, --seed), divide the survivors by
1 - drop rate, add them up with --weights, add --scaling times the result to the base
(storage.dare_merge_from_artifacts).  --drop-rate 0 is task arithmetic.  The task models are never written: the values
are formed in one pass over the stored bases.  For stores of unmasked runs (masks are not stored, reload.py:204-205).
Prints the kept counts as a JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="DARE merge / task arithmetic of stored SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--base-model-path", required=True, help="Path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Path to save the merged model (default: not written)")
    ap.add_argument("--drop-rate", type=float, default=0.9,
                    help="Probability that a value of a task vector is dropped, in [0, 1); 0 = task arithmetic "
                         "(default 0.9)")
    ap.add_argument("--seed", type=int, default=0, help="Seed of the mask, in [0, 2^64) (default 0)")
    ap.add_argument("--no-rescale", action="store_true", help="Do not divide the kept values by 1 - drop rate")
    ap.add_argument("--weights", nargs="+", type=float, default=None,
                    help="One weight per merged task, in sorted task-name order (default: 1.0 each)")
    ap.add_argument("--normalize", action="store_true", help="Divide the weights by their sum")
    ap.add_argument("--scaling", type=float, default=1.0, help="Factor on the merged task vector (default 1.0)")
    ap.add_argument("--tasks", nargs="+", default=None, help="Task names to merge (default: every stored task)")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    for what, path in (("--artifact-dir", args.artifact_dir), ("--base-model-path", args.base_model_path)):
        if not os.path.exists(path):
            ap.error(f"{what}: {path} does not exist")
    if not 0.0 <= args.drop_rate < 1.0:
        ap.error(f"--drop-rate: {args.drop_rate} is outside [0, 1)")
    if not 0 <= args.seed < 1 << 64:
        ap.error(f"--seed: {args.seed} is outside [0, 2^64)")
    from svdq_amd.storage import dare_merge_from_artifacts, load_all_artifacts
    weights = None
    if args.weights is not None:
        names = args.tasks
        if names is None:
            names = {t for per_task in load_all_artifacts(args.artifact_dir, device="cpu")["compressed"].values()
                     for t in per_task}
        names = sorted(set(names))
        if len(args.weights) != len(names):
            ap.error(f"--weights: {len(args.weights)} values for the {len(names)} tasks {names}")
        weights = dict(zip(names, args.weights))
    res = dare_merge_from_artifacts(args.artifact_dir, args.base_model_path, args.output_path, drop_rate=args.drop_rate,
                                    seed=args.seed, rescale=not args.no_rescale, weights=weights,
                                    normalize=args.normalize, scaling=args.scaling, tasks=args.tasks, device=args.device)
    stats = res["stats"]
    print(json.dumps({"kept": stats["kept"]}))
    print(json.dumps({"rows": stats["rows"], "drop_threshold": stats["drop_threshold"]}))
    where = f" -> {args.output_path}" if args.output_path else ""
    print(f"merged {len(res['merged_state_dict'])} entries{where}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
