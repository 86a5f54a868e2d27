"""
The command line with --eval-from-checkpoints: a run with reconstruction diagnostics that never forms the task vectors
(compression through svdq_compress_from_base, Step 8 through svdq_diagnostics_from_base) gives the diagnostics, the
merged model and the artifact files of the ordinary run.
"""
import json
import os

import numpy as np
import pytest
import torch

from helpers import artifact_manifest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sq():
    import svdq_amd
    return svdq_amd


def _write_checkpoints(tmp, tasks, with_masks):
    """The tiny checkpoints of tests/test_hip_cli.py."""
    from oracle.svd_hybrid_oracle import synthetic_deltas
    g = torch.Generator().manual_seed(123)
    shapes = {"blk.attn.weight": (96, 64), "blk.attn.bias": (96,), "blk.mlp.weight": (128, 64), "ln.weight": (64,)}
    base = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    base["steps"] = torch.tensor(7)
    ck = tmp / "ckpt"
    ck.mkdir()
    torch.save({"state_dict": base}, tmp / "base.pt")
    deltas = {k: synthetic_deltas(int(np.prod(s)), len(tasks), 700 + i) for i, (k, s) in enumerate(shapes.items())}
    for ti, t in enumerate(tasks):
        sd = {k: base[k] + deltas[k][ti].view(shapes[k]) for k in shapes}
        sd["steps"] = torch.tensor(9)
        torch.save(sd, ck / f"{t}.pt")
    if with_masks:
        md = tmp / "masks"
        md.mkdir()
        for t in tasks:
            torch.save({"blk.mlp.weight": torch.rand(shapes["blk.mlp.weight"], generator=g) > 0.6}, md / f"{t}_mask.pt")
    return shapes


def _same_tree(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), path
        for k in a:
            _same_tree(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f"{path}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), path
    elif isinstance(a, float) and a != a:
        assert b != b, path
    else:
        assert a == b, (path, a, b)


def _same_files(d1, d2):
    """The same files with the same contents (tensors byte for byte); the two runs' own directory names aside."""
    man = artifact_manifest(d1)
    assert man == artifact_manifest(d2) and man
    for rel in man:
        f1, f2 = os.path.join(d1, rel), os.path.join(d2, rel)
        if rel.endswith(".pt"):
            _same_tree(torch.load(f1, map_location="cpu", weights_only=True),
                       torch.load(f2, map_location="cpu", weights_only=True), rel)
        else:
            j1, j2 = json.load(open(f1)), json.load(open(f2))
            for j in (j1, j2):
                for key in ("output_dir", "artifact_dir"):
                    j.pop(key, None)
            _same_tree(j1, j2, rel)


@pytest.mark.parametrize("with_masks", [False, True])
def test_eval_from_checkpoints_matches_the_ordinary_run(sq, tmp_path, monkeypatch, with_masks):
    tasks = ["Cars", "DTD", "EuroSAT", "GTSRB", "MNIST", "SVHN"]
    shapes = _write_checkpoints(tmp_path, tasks, with_masks)
    common = ["--tasks", *tasks, "--checkpoint-dir", str(tmp_path / "ckpt"), "--base-model-path", str(tmp_path / "base.pt"),
              "--energy-threshold", "0.9", "--max-rank", "2", "--store-artifacts"]
    if with_masks:
        common += ["--mask-dir", str(tmp_path / "masks"), "--include-noise"]
    a = sq.cli.main(common + ["--output-dir", str(tmp_path / "o1"), "--artifact-dir", str(tmp_path / "a1")])

    def no_task_vectors(*args, **kwargs):
        raise AssertionError("the flagged run must not form task vectors")
    monkeypatch.setattr(sq.cli, "load_task_vectors", no_task_vectors)
    b = sq.cli.main(common + ["--eval-from-checkpoints", "--output-dir", str(tmp_path / "o2"), "--artifact-dir",
                              str(tmp_path / "a2")])
    assert sorted(a["diagnostics"]["per_parameter"]) == sorted(shapes)
    _same_tree(a["diagnostics"], b["diagnostics"])
    for n in shapes:
        assert list(a["diagnostics"]["per_parameter"][n]["reconstruction_errors"]) == tasks
    assert set(a["merged_state_dict"]) == set(b["merged_state_dict"])
    for k in a["merged_state_dict"]:
        assert torch.equal(a["merged_state_dict"][k].cpu(), b["merged_state_dict"][k].cpu()), k
    m1 = torch.load(tmp_path / "o1" / "merged_state_dict.pt", map_location="cpu", weights_only=True)
    m2 = torch.load(tmp_path / "o2" / "merged_state_dict.pt", map_location="cpu", weights_only=True)
    assert all(torch.equal(m1[k], m2[k]) for k in m1) and set(m1) == set(m2)
    _same_files(str(tmp_path / "a1"), str(tmp_path / "a2"))
