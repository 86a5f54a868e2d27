#!/usr/bin/env python3
"""Merge a stored artifact set again under another weighting (compute_weights weighting.py:266-329, cluster_tasks
clustering.py:198-245, merge_with_clustering merge.py:555-626) from the artifact directory and the base checkpoint alone:
the fine-tuned checkpoints are not needed.  --weighting cluster clusters the tasks on the Gram of what the store
reconstructs, one pass over the stored bases (storage.remerge_from_artifacts).  Without --weighting the stored weights are
used, which is load_and_merge.py.  Exact for stores of unmasked runs (masks are not stored, reload.py:204-205)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="Re-merge stored SVD-Hybrid artifacts under another task weighting")
    ap.add_argument("--artifact-dir", required=True, help="Directory containing artifacts")
    ap.add_argument("--base-model-path", required=True, help="Path to base model checkpoint")
    ap.add_argument("--output-path", default=None, help="Path to save the merged model (default: not written)")
    ap.add_argument("--weighting", default=None, choices=["uniform", "performance", "cluster"],
                    help="Task weighting strategy (default: the weights stored in diagnostics.json)")
    ap.add_argument("--cluster-k", type=int, default=None,
                    help="Number of clusters for --weighting cluster (default: the stored configuration's)")
    ap.add_argument("--performance-file", default=None, help="Path to performance metrics JSON file")
    ap.add_argument("--temperature", type=float, default=None,
                    help="Temperature for performance-based weighting (default: the stored configuration's)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--update-store", action="store_true",
                    help="also rewrite diagnostics.json (task_weights, cluster_assignments) and clusters.json in the store")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    for what, path in (("--artifact-dir", args.artifact_dir), ("--base-model-path", args.base_model_path),
                       ("--performance-file", args.performance_file)):
        if path is not None and not os.path.exists(path):
            ap.error(f"{what}: {path} does not exist")
    from svdq_amd.storage import remerge_from_artifacts
    res = remerge_from_artifacts(args.artifact_dir, args.base_model_path, args.output_path, weighting=args.weighting,
                                 cluster_k=args.cluster_k, performance_file=args.performance_file,
                                 temperature=args.temperature, device=args.device, update_store=args.update_store)
    print("weights: " + json.dumps(res["weights"]))
    if res["cluster_assignments"] is not None:
        print("clusters: " + json.dumps(res["cluster_assignments"]))
    where = f" -> {args.output_path}" if args.output_path else ""
    print(f"merged {len(res['merged_state_dict'])} entries{where}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
