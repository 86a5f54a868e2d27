#!/usr/bin/env python3
"""The EMR merge (Huang et al. 2024, "EMR-Merging") of a stored artifact set, in two steps.

Step 1, from the artifact directory alone (storage.emr_from_artifacts): one elected task vector, a 1-bit mask per task
and one rescaler per task, written to --output-dir as emr_unified.pt, EMR_mask_{T}task.npz and emr_rescalers.json.  The
task models are never written: the values are formed in one pass over the stored bases.  Nothing is tuned.

    emr_merge.py --artifact-dir ART --output-dir OUT [--tasks A B ...]

Step 2, from those files and the base checkpoint (storage.emr_task_model_from_files): task NAME's model
base + rescaler * (mask ? elected : 0), in one launch over the model.

    emr_merge.py --output-dir OUT --task NAME --base-model-path BASE --output-path MODEL

For stores of unmasked runs (masks are not stored, reload.py:204-205).  Step 1 prints the rescalers and the set bits
per task as JSON lines, step 2 the rescaler it applied."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="EMR merge of stored SVD-Hybrid artifacts, and a task's model from it")
    ap.add_argument("--artifact-dir", default=None, help="Directory containing artifacts (step 1)")
    ap.add_argument("--output-dir", required=True, help="Directory of the EMR files: written by step 1, read by step 2")
    ap.add_argument("--tasks", nargs="+", default=None, help="Task names to merge (default: every stored task)")
    ap.add_argument("--task", default=None, help="Step 2: the task whose model is formed")
    ap.add_argument("--base-model-path", default=None, help="Step 2: path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Step 2: path to save the task's model")
    ap.add_argument("--rescale", type=float, default=None, help="Step 2: a scalar in place of the task's stored rescaler")
    ap.add_argument("--device", default="cuda")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.task is None:
        if args.artifact_dir is None:
            ap.error("give --artifact-dir (step 1) or --task with --base-model-path (step 2)")
        if not os.path.exists(args.artifact_dir):
            ap.error(f"--artifact-dir: {args.artifact_dir} does not exist")
        from svdq_amd.storage import emr_from_artifacts
        res = emr_from_artifacts(args.artifact_dir, args.output_dir, tasks=args.tasks, device=args.device)
        print(json.dumps({"rescalers": res["rescalers"]}))
        print(json.dumps({"active": res["stats"]["active"], "rows": res["stats"]["rows"]}))
        print(f"elected {len(res['unified'])} parameters for {len(res['rescalers'])} tasks -> {args.output_dir}")
        return 0
    if args.base_model_path is None or args.output_path is None:
        ap.error("--task needs --base-model-path and --output-path")
    for what, path in (("--output-dir", args.output_dir), ("--base-model-path", args.base_model_path)):
        if not os.path.exists(path):
            ap.error(f"{what}: {path} does not exist")
    if args.rescale is not None and not (args.rescale == args.rescale and abs(args.rescale) != float("inf")):
        ap.error(f"--rescale: {args.rescale} is not a finite number")
    from svdq_amd.storage import emr_task_model_from_files
    res = emr_task_model_from_files(args.output_dir, args.task, args.base_model_path, args.output_path,
                                    rescale=args.rescale, device=args.device)
    print(json.dumps({"task": args.task, "rescaler": res["rescaler"]}))
    print(f"task model of {len(res['state_dict'])} entries -> {args.output_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
