#!/usr/bin/env python3
"""TALL masks and the consensus merge (Wang et al. 2024) of a stored artifact set, from the artifact directory and the
base checkpoint alone: task t's mask is |v_t| > lambda * |sum of the other tasks' values| (--tall-lambda), a row of the
summed task vector is kept where at least --k masks are set, and --scaling times the result is added to the base
(storage.consensus_merge_from_artifacts).  --k 0 is task arithmetic.  --mask-output writes the bit-packed per-task masks
as an .npz; named TALL_mask_{T}task.npz inside a directory, a later run reads it through --mask-dir with the same base.
The task models are never written: the values are formed in one pass over the stored bases.  For stores of unmasked
runs (masks are not stored, reload.py:204-205).  Prints the set bits per task and the agreement histogram as JSON
lines."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="TALL masks and consensus merge of stored SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--base-model-path", required=True, help="Path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Path to save the merged model (default: not written)")
    ap.add_argument("--mask-output", default=None,
                    help="Path of the .npz that receives the packed per-task masks (default: not written)")
    ap.add_argument("--tall-lambda", type=float, default=0.4,
                    help="A value is in its task's mask iff |v_t| > lambda * |sum of the other tasks| (default 0.4)")
    ap.add_argument("--k", type=int, default=2,
                    help="Rows kept: at least k masks set; 0 = task arithmetic, at most the task count (default 2)")
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
    if not (args.tall_lambda >= 0.0 and args.tall_lambda != float("inf")):
        ap.error(f"--tall-lambda: {args.tall_lambda} is not a finite number >= 0")
    if args.k < 0:
        ap.error(f"--k: {args.k} is negative")
    from svdq_amd.storage import consensus_merge_from_artifacts
    res = consensus_merge_from_artifacts(args.artifact_dir, args.base_model_path, args.output_path,
                                         mask_output_path=args.mask_output, tall_lambda=args.tall_lambda, k=args.k,
                                         scaling=args.scaling, tasks=args.tasks, device=args.device)
    stats = res["stats"]
    print(json.dumps({"active": stats["active"]}))
    print(json.dumps({"agreement": stats["agreement"], "rows": stats["rows"]}))
    where = f" -> {args.output_path}" if args.output_path else ""
    masks = f", masks -> {args.mask_output}" if args.mask_output else ""
    print(f"merged {len(res['merged_state_dict'])} entries{where}{masks}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
