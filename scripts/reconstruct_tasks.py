#!/usr/bin/env python3
"""Write every task's own model back out of stored artifacts: <output-dir>/<task>.pt = base + that task's reconstructed
task vector (reconstruct_from_coefficients merge.py:144-194 per task, apply_merged_deltas merge.py:429-552), all tasks
of a plan in one pass over its basis.  The original fine-tuned checkpoints are not needed."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Reconstruct per-task models from SVD-Hybrid artifacts")
    ap.add_argument("--artifact-dir", required=True)
    ap.add_argument("--base-model-path", required=True)
    ap.add_argument("--tasks", nargs="+", default=None, help="task names (default: every task of the artifacts)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    from svdq_amd.storage import reconstruct_tasks_from_artifacts
    models = reconstruct_tasks_from_artifacts(args.artifact_dir, args.base_model_path, tasks=args.tasks,
                                              output_dir=args.output_dir, device=args.device)
    for t, sd in models.items():
        print(f"{t}: {len(sd)} entries -> {os.path.join(args.output_dir, t.replace('/', '_'))}.pt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
