#!/usr/bin/env python3
"""Add new fine-tuned checkpoints to a stored artifact set: each is projected onto the bases already stored
(project_to_basis compress.py:6-21 inside compress_all_parameters compress.py:173-207, for the new tasks alone), its
coefficients are quantized and written beside the other tasks'.  The other tasks' checkpoints are not needed and no basis
is recomputed; afterwards load_and_merge.py / reconstruct_tasks.py see one more task.  --extend-basis also grows the
stored bases by the directions the new tasks add outside their span (storage.add_tasks_to_artifacts).  --weighting
cluster then clusters ALL tasks, old and new, on the Gram of what the enlarged store reconstructs (cluster_tasks
clustering.py:198-245 through storage.remerge_from_artifacts) and writes the cluster weights and labels into the store.

A store that was compressed through masks needs the mask directory the run had (--mask-dir): masks are not stored
(reload.py:204-205)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="Add fine-tuned checkpoints to stored SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True)
    ap.add_argument("--base-model-path", required=True)
    ap.add_argument("--checkpoint", action="append", required=True, metavar="NAME=PATH",
                    help="a new task and its fine-tuned checkpoint; repeat for several")
    ap.add_argument("--mask-dir", default=None,
                    help="directory of the task masks the store was compressed with (needed for a masked store)")
    ap.add_argument("--output-dir", default=None, help="where the enlarged store goes (default: in place)")
    ap.add_argument("--weights-json", default=None,
                    help="JSON file {task: weight} over ALL tasks, old and new (default: uniform)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--extend-basis", action="store_true",
                    help="also grow the stored bases by the directions the new tasks add outside their span "
                         "(1 to 8 new tasks; without it a new task reconstructs little more than the stored mean)")
    ap.add_argument("--min-residual", type=float, default=2.0 ** -12,
                    help="with --extend-basis: keep a residual direction whose norm exceeds this share of the largest "
                         "centred task norm (default 2^-12)")
    ap.add_argument("--weighting", default=None, choices=["cluster"],
                    help="after adding: cluster all tasks on what the store reconstructs and store the cluster weights "
                         "(diagnostics.json task_weights / cluster_assignments, clusters.json); default: --weights-json "
                         "or uniform, as before")
    ap.add_argument("--cluster-k", type=int, default=None,
                    help="with --weighting cluster: number of clusters (default: the stored configuration's)")
    return ap


def parse_checkpoints(ap, items):
    """NAME=PATH pairs -> {name: path}, in the order given; malformed or repeated names end the run (argparse error)."""
    out = {}
    for item in items:
        name, sep, path = item.partition("=")
        if not sep or not name or not path:
            ap.error(f"--checkpoint takes NAME=PATH, got {item!r}")
        if name in out:
            ap.error(f"--checkpoint names task {name!r} twice")
        out[name] = path
    return out


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    checkpoints = parse_checkpoints(ap, args.checkpoint)
    for what, path in [("--base-model-path", args.base_model_path)] + [(f"--checkpoint {n}", p) for n, p in checkpoints.items()]:
        if not os.path.exists(path):
            ap.error(f"{what}: {path} does not exist")
    weights = None
    if args.weights_json is not None:
        with open(args.weights_json) as f:
            weights = json.load(f)
        if not isinstance(weights, dict):
            ap.error("--weights-json must hold one JSON object {task: weight}")
    from svdq_amd.storage import _load_base, add_tasks_to_artifacts
    base, masks = args.base_model_path, None
    if args.mask_dir is not None:
        from reconstruct_tasks import load_combined_masks
        base = _load_base(args.base_model_path, args.device)
        masks = load_combined_masks(args.artifact_dir, base, args.mask_dir, None, args.device)
    res = add_tasks_to_artifacts(args.artifact_dir, base, checkpoints, masks=masks, output_dir=args.output_dir,
                                 weights=weights, device=args.device, extend_basis=args.extend_basis,
                                 min_residual=args.min_residual)
    print(f"added {res['added']} -> {res['output_dir']}: {len(res['tasks'])} tasks, "
          f"{len(res['compressed'])} parameters projected")
    if args.extend_basis:
        print(f"new basis columns: {sum(res['columns'].values())} over {len(res['columns'])} entries; energy the stored "
              f"columns captured: " + ", ".join(f"{t} {e:.4f}" for t, e in res["captured_energy"].items()))
    if args.weighting == "cluster":
        from svdq_amd.storage import remerge_from_artifacts
        rem = remerge_from_artifacts(res["output_dir"], base, None, weighting="cluster", cluster_k=args.cluster_k,
                                     device=args.device, update_store=True)
        print("clusters: " + json.dumps(rem["cluster_assignments"]))
        print("weights: " + json.dumps(rem["weights"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
