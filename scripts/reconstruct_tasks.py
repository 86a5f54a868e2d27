#!/usr/bin/env python3
"""Write every task's own model back out of stored artifacts: <output-dir>/<task>.pt = base + that task's reconstructed
task vector (reconstruct_from_coefficients merge.py:144-194 per task, apply_merged_deltas merge.py:429-552), all tasks
of a plan in one pass over its basis.  The original fine-tuned checkpoints are not needed.

A run that compressed through masks stored compacted rows and no masks (reload.py:204-205): give it the mask directory
the run had (--mask-dir, and --mask-strategy when it differs from the stored configuration) and the rows go back at
their source positions inside the streaming launch (reconstruct_from_masked mask_loader.py:712-763)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser():
    ap = argparse.ArgumentParser(description="Reconstruct per-task models from SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True)
    ap.add_argument("--base-model-path", required=True)
    ap.add_argument("--tasks", nargs="+", default=None, help="task names (default: every task of the artifacts)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--mask-dir", default=None,
                    help="directory of the task masks the run compressed with (needed for a masked run)")
    ap.add_argument("--mask-strategy", default=None, choices=["union", "intersection", "majority"],
                    help="how the task masks were combined (default: the stored configuration's)")
    return ap


def load_combined_masks(artifact_dir, base, mask_dir, strategy, device):
    """The combined masks of the run, as cli.py builds them: load_task_masks over ALL the run's tasks, combine_masks."""
    from svdq_amd.mask_loader import combine_masks, load_task_masks
    from svdq_amd.storage import load_config
    config = load_config(artifact_dir)
    task_masks = load_task_masks(mask_dir, list(config.tasks), device=device, reference_state_dict=base)
    return combine_masks(task_masks, strategy=strategy or config.svd_mask_strategy, device=device, verbose=False)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.mask_strategy is not None and args.mask_dir is None:
        ap.error("--mask-strategy needs --mask-dir")
    from svdq_amd.storage import _load_base, reconstruct_tasks_from_artifacts_masked
    base, masks = args.base_model_path, None
    if args.mask_dir is not None:
        base = _load_base(args.base_model_path, args.device)
        masks = load_combined_masks(args.artifact_dir, base, args.mask_dir, args.mask_strategy, args.device)
    models = reconstruct_tasks_from_artifacts_masked(args.artifact_dir, base, masks, tasks=args.tasks,
                                                     output_dir=args.output_dir, device=args.device,
                                                     fused_masks=masks is not None)
    for t, sd in models.items():
        print(f"{t}: {len(sd)} entries -> {os.path.join(args.output_dir, t.replace('/', '_'))}.pt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
