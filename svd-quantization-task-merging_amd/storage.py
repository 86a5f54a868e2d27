"""
Artifact writer / reader with the reference's on-disk format (reference
src/svd_hybrid/storage.py:52-409, reload.py:142-238):

    <artifact_dir>/basis/<safe_name>.pt    {"masked"|"noise": {U_high, U_low, singular_values, k, mean,
                                                                energy_retained, D, N}}          CPU tensors
    <artifact_dir>/coeffs/<safe_name>.pt   {task: {"masked"|"unmasked": {c_high_fp16, c_low_quant}}}
    <artifact_dir>/diagnostics.json, config.json
    <output_dir>/merged_state_dict.pt

safe_name = name.replace("/", "_").replace("\\\\", "_") (storage.py:72).  Pure host code: tensors are moved
to the CPU and written with torch.save, exactly as the reference does; the private keys this package
attaches to basis dicts (fused-run bookkeeping) are not written.
"""
from __future__ import annotations

import json
import os
from dataclasses import asdict
from typing import Any, Dict, Optional

import torch

_BASIS_KEYS = ("U_high", "U_low", "singular_values", "k", "mean", "energy_retained", "D", "N")


def _safe(name: str) -> str:
    return name.replace("/", "_").replace("\\", "_")


def _compact(obj):
    """Deep copy in which every tensor owns exactly its own elements: the payload tensors handed out by the
    batched path are views into one packed host buffer, and torch.save writes a view's WHOLE storage."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _compact(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and not isinstance(obj, torch.Size):
        return type(obj)(_compact(v) for v in obj)
    return obj


def _basis_payload(b: Dict) -> Dict:
    return {"U_high": b["U_high"].cpu(), "U_low": b["U_low"].cpu(), "singular_values": b["singular_values"].cpu(),
            "k": b["k"], "mean": b["mean"].cpu() if b["mean"] is not None else None,
            "energy_retained": b["energy_retained"], "D": b["D"], "N": b["N"]}


def save_basis(basis: Dict, param_name: str, output_dir: str):
    """Reference storage.py:52-106."""
    d = os.path.join(output_dir, "basis")
    os.makedirs(d, exist_ok=True)
    data = {}
    if basis.get("masked") is not None:
        data["masked"] = _basis_payload(basis["masked"])
    if basis.get("noise") is not None:
        data["noise"] = _basis_payload(basis["noise"])
    torch.save(data, os.path.join(d, f"{_safe(param_name)}.pt"))


def load_basis(param_name: str, artifact_dir: str, device: str = "cpu") -> Dict:
    """Reference storage.py:109-134 (files written by save_basis hold tensors and plain scalars only)."""
    path = os.path.join(artifact_dir, "basis", f"{_safe(param_name)}.pt")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Basis file not found: {path}")
    return torch.load(path, map_location=device, weights_only=True)   # tensors, scalars, None, dict: nothing executes


def save_compressed_coefficients(compressed: Dict[str, Dict[str, Dict]], output_dir: str):
    """Reference storage.py:137-174."""
    d = os.path.join(output_dir, "coeffs")
    os.makedirs(d, exist_ok=True)
    for name, per_task in compressed.items():
        out = {}
        for task, art in per_task.items():
            a = {}
            for region in ("masked", "unmasked"):
                if art.get(region) is not None:
                    a[region] = {"c_high_fp16": _compact(art[region]["c_high_fp16"]),
                                 "c_low_quant": _compact(art[region]["c_low_quant"])}
            out[task] = a
        torch.save(out, os.path.join(d, f"{_safe(name)}.pt"))


def load_compressed_coefficients(param_name: str, artifact_dir: str, device: str = "cpu") -> Dict[str, Dict]:
    """Reference storage.py:177-202."""
    path = os.path.join(artifact_dir, "coeffs", f"{_safe(param_name)}.pt")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Coefficients file not found: {path}")
    # tensors, int / float / str / None, dict / list and torch.Size only: the weights-only unpickler accepts all of it
    return torch.load(path, map_location=device, weights_only=True)


def _serializable(obj):
    if isinstance(obj, dict):
        return {k: _serializable(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_serializable(v) for v in obj]
    if isinstance(obj, torch.Size):
        return list(obj)
    if isinstance(obj, torch.Tensor):
        return obj.cpu().tolist() if obj.numel() > 1 else obj.item()
    if hasattr(obj, "item"):
        return obj.item()
    return obj


def save_diagnostics(diagnostics: Dict[str, Any], output_dir: str):
    """Reference storage.py:205-237."""
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "diagnostics.json"), "w") as f:
        json.dump(_serializable(diagnostics), f, indent=2)


def load_diagnostics(artifact_dir: str) -> Dict[str, Any]:
    """Reference storage.py:240-258."""
    path = os.path.join(artifact_dir, "diagnostics.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Diagnostics file not found: {path}")
    with open(path) as f:
        return json.load(f)


def save_config(config, output_dir: str):
    """Reference storage.py:261-280."""
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "config.json"), "w") as f:
        d = asdict(config)
        # the key set must be exactly the reference dataclass's: its load_config does SVDHybridConfig(**json)
        # (storage.py:283-303) and raises TypeError on anything else.  The mixed-width extension is a function of
        # the parameter name and not serialisable anyway; the widths actually used are in every coeffs/*.pt
        # ("c_low_quant"["num_bits"]).
        d.pop("svd_low_bits_by_param", None)
        json.dump(d, f, indent=2)


def load_config(artifact_dir: str):
    """Reference storage.py:283-303."""
    from .config import SVDHybridConfig
    path = os.path.join(artifact_dir, "config.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Config file not found: {path}")
    with open(path) as f:
        return SVDHybridConfig(**json.load(f))


def save_all_artifacts(bases: Dict[str, Dict], compressed: Dict[str, Dict[str, Dict]], diagnostics: Dict[str, Any],
                       config, output_dir: str):
    """Reference storage.py:306-338."""
    for name, basis in bases.items():
        save_basis(basis, name, output_dir)
    save_compressed_coefficients(compressed, output_dir)
    save_diagnostics(diagnostics, output_dir)
    save_config(config, output_dir)


def load_all_artifacts(artifact_dir: str, device: str = "cpu") -> Dict[str, Any]:
    """Reference storage.py:341-389: the parameter list comes from diagnostics["per_parameter"]."""
    config = load_config(artifact_dir)
    diagnostics = load_diagnostics(artifact_dir)
    names = list(diagnostics.get("per_parameter", {}).keys())
    bases, compressed = {}, {}
    for n in names:
        try:
            bases[n] = load_basis(n, artifact_dir, device)
        except FileNotFoundError:
            pass
        try:
            compressed[n] = load_compressed_coefficients(n, artifact_dir, device)
        except FileNotFoundError:
            pass
    return {"bases": bases, "compressed": compressed, "diagnostics": diagnostics, "config": config}


def save_merged_model(merged_state_dict: Dict[str, torch.Tensor], output_dir: str,
                      filename: str = "merged_state_dict.pt"):
    """Reference storage.py:392-409."""
    os.makedirs(output_dir, exist_ok=True)
    torch.save(merged_state_dict, os.path.join(output_dir, filename))


def reconstruct_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None, device: str = "cpu") -> Dict:
    """Reference reload.py:142-238: rebuild the merged model from stored artifacts.  Masks are not stored
    (reload.py:204-205), so this is exact for unmasked runs only -- as in the reference.
    ``base_model_path`` may also be an already-loaded state dict."""
    from .merge import apply_merged_deltas, merge_all_parameters
    from .driver import adopt_artifacts
    art = load_all_artifacts(artifact_dir, device=device)
    config, diagnostics = art["config"], art["diagnostics"]
    # into plans: the merge below then takes two launches per plan (svdq_plan_import + svdq_merge) instead of a payload
    # upload, a dequantize and a reconstruct launch per (parameter, task); what adoption declines stays as loaded
    bases, compressed = adopt_artifacts(art.pop("bases"), art.pop("compressed"), config, device=device)
    tasks = list(diagnostics.get("task_weights", {}).keys())
    if not tasks:
        tasks = list(next(iter(compressed.values())).keys())
    weights = diagnostics.get("task_weights") or {t: 1.0 / len(tasks) for t in tasks}
    shapes = {n: torch.Size(d["original_shape"]) for n, d in diagnostics.get("per_parameter", {}).items()
              if d.get("original_shape") is not None}
    merged = merge_all_parameters(compressed, bases, {}, weights, shapes, config, device=device, verbose=False)
    base = _load_base(base_model_path, device)
    out = apply_merged_deltas(base, merged, device=device, verbose=False)
    if output_path:
        torch.save(out, output_path)
    return {"merged_state_dict": out, "diagnostics": diagnostics, "config": config}


def _load_base(base_model_path, device):
    """A base state dict from a path (wrappers unwrapped as task_vector_loader.py does) or as given."""
    if isinstance(base_model_path, dict):
        return base_model_path
    base = torch.load(base_model_path, map_location=device, weights_only=True)
    for key in ("state_dict", "model", "model_state_dict"):
        if isinstance(base, dict) and key in base and isinstance(base[key], dict):
            return base[key]
    return base


def reconstruct_tasks_from_artifacts(artifact_dir: str, base_state_dict, tasks=None, output_dir: str = None,
                                     device: str = "cuda") -> Dict[str, Dict[str, torch.Tensor]]:
    """Every task's own model back out of stored artifacts of an UNMASKED run (masks are not stored, reload.py:204-205):
    ``reconstruct_tasks_from_artifacts_masked`` without masks, which see."""
    return reconstruct_tasks_from_artifacts_masked(artifact_dir, base_state_dict, None, tasks=tasks, output_dir=output_dir,
                                                   device=device, fused_masks=False)


def reconstruct_tasks_from_artifacts_masked(artifact_dir: str, base_state_dict, masks: Optional[Dict[str, torch.Tensor]],
                                            tasks=None, output_dir: str = None, device: str = "cuda",
                                            fused_masks: bool = True) -> Dict[str, Dict[str, torch.Tensor]]:
    """Every task's own model back out of stored artifacts: {task: state dict} with ``base + delta_task`` for the
    parameters the artifacts cover and a clone of the base tensor for the others (as apply_merged_deltas does).
    load_all_artifacts -> adopt_artifacts -> merge.reconstruct_task_vectors: two launches per plan for all tasks.  Masks
    are not stored (reload.py:204-205): without ``masks`` this is exact for unmasked runs only, like
    ``reconstruct_from_artifacts``; a masked run needs the combined masks it compressed with ({parameter: mask}, on
    ``device``), and with ``fused_masks`` the rows go back at their source positions inside the streaming launch
    (svdq_task_reconstruct_masked) wherever a mask selects exactly the stored rows.
    ``base_state_dict``: a state dict or the path of one; ``tasks``: names (None = all); with ``output_dir`` each
    task's state dict is written to ``<output_dir>/<task>.pt``."""
    from .merge import reconstruct_task_vectors_masked
    from .driver import adopt_artifacts
    art = load_all_artifacts(artifact_dir, device=device)
    config, diagnostics = art["config"], art["diagnostics"]
    if tasks is not None:      # before any device work
        known = {t for per_task in art["compressed"].values() for t in per_task}
        for t in tasks:
            if t not in known:
                raise ValueError(f"unknown task {t!r}: the artifacts hold {sorted(known)}")
    base = _load_base(base_state_dict, device)
    masks = masks or {}
    bases, compressed = adopt_artifacts(art.pop("bases"), art.pop("compressed"), config, device=device,
                                        masks=masks if fused_masks else None)
    shapes = {n: torch.Size(d["original_shape"]) for n, d in diagnostics.get("per_parameter", {}).items()
              if d.get("original_shape") is not None}
    covered = {n: b for n, b in base.items() if n in compressed}
    models = reconstruct_task_vectors_masked(compressed, bases, masks, shapes, config, tasks=tasks, device=device,
                                             base_state_dict=covered, fused_masks=fused_masks)
    out = {}
    for t, params in models.items():
        out[t] = {n: (params[n] if n in params else b.clone()) for n, b in base.items()}
        if output_dir:
            save_merged_model({n: v.cpu() for n, v in out[t].items()}, output_dir, filename=f"{_safe(t)}.pt")
    return out


def _stored_tasks(compressed: Dict[str, Dict], diagnostics: Dict[str, Any]) -> list:
    """The task names a store holds, in the order of its weights, then of first appearance in the coefficient files."""
    tasks = list((diagnostics.get("task_weights") or {}).keys())
    for per_task in compressed.values():
        for t in per_task:
            if t not in tasks:
                tasks.append(t)
    return tasks


def add_tasks_to_artifacts(artifact_dir: str, base_state_dict, finetuned: Dict[str, Any],
                           masks: Optional[Dict[str, torch.Tensor]] = None, output_dir: str = None,
                           weights: Optional[Dict[str, float]] = None, device: str = "cuda",
                           extend_basis: bool = False, min_residual: float = 2.0 ** -12) -> Dict[str, Any]:
    """Add NEW fine-tuned models to a stored artifact set: each is projected onto the bases already stored, its
    coefficients are quantized and it joins the per-parameter coefficient dictionaries -- compress_all_parameters
    (reference compress.py:173-207) for the new tasks alone.  The other tasks' checkpoints are not needed and no basis is
    recomputed.  load_all_artifacts -> compress.project_all_parameters (one svdq_plan_project per plan, finetuned - base
    formed inside the launch: no task vectors are materialised) -> the existing writers.

    ``base_state_dict`` / the values of ``finetuned`` ({task: checkpoint}): state dicts or paths of them.  ``masks``:
    the combined masks the store was compressed with ({parameter: mask}; masks are not stored, reload.py:204-205).
    ``weights``: {task: weight} over ALL tasks, old and new, for ``diagnostics["task_weights"]``; None = uniform over all.
    ``output_dir``: None or the artifact directory itself = in place, and then only the coefficient files and
    diagnostics.json are rewritten; any other directory receives the whole store.
    A task name the store already holds, or more than 32 tasks in total, is a ``ValueError`` before anything is read
    from the checkpoints.  Returns {"tasks", "added", "compressed" (the new tasks' artifacts), "output_dir"}.

    ``extend_basis=True`` (1 to 8 new tasks): the stored U_high of every batched entry also grows by the orthonormal
    directions the new tasks add outside the span of the stored columns (``compress.extend_bases``; ``min_residual`` is
    its threshold) -- without it a new task's artifact reconstructs little more than the stored mean, since r <= N
    stored directions span next to nothing of a new delta.  The old tasks' ``c_high`` of extended entries are zero-padded
    (their reconstructions do not move), the extended basis files are written as well, and ``captured_energy`` ({task:
    share of its energy the stored columns captured}) and ``columns`` ({"param [region]": new columns}) go into
    diagnostics.json and the return value.  ``False`` is the plain route, bit for bit."""
    from . import _native as nat
    from .compress import check_extension_room, extend_bases, pad_c_high, project_all_parameters
    art = load_all_artifacts(artifact_dir, device="cpu")
    config, diagnostics, bases, compressed = art["config"], art["diagnostics"], art["bases"], art["compressed"]
    old = _stored_tasks(compressed, diagnostics)
    new = list(finetuned.keys())
    if not new:
        raise ValueError("no checkpoint to add")
    for t in new:
        if t in old:
            raise ValueError(f"task {t!r} is already in the artifacts, which hold {old}")
    if len(old) + len(new) > nat.MAX_TASKS:
        raise ValueError(f"{len(old)} stored + {len(new)} new tasks: at most {nat.MAX_TASKS} tasks in total")
    if extend_basis:
        check_extension_room(bases, len(new), len(old))
    tasks = old + new
    if weights is not None:
        lacking = [t for t in tasks if t not in weights]
        if lacking:
            raise ValueError(f"weights lack task {lacking[0]!r}: they must cover all {len(tasks)} tasks")
        task_weights = {t: float(weights[t]) for t in tasks}
    else:
        task_weights = {t: 1.0 / len(tasks) for t in tasks}
    base = _load_base(base_state_dict, device)
    models = {}
    for t, ckpt in finetuned.items():
        sd = _load_base(ckpt, device)
        models[t] = {n: sd[n] for n in bases if n in sd and n in base}
    base_sd = {n: base[n] for n in bases if n in base}
    extension, grown = None, {}
    if extend_basis:
        extension = extend_bases(models, masks or {}, bases, config, device=device, base_state_dict=base_sd,
                                 min_residual=min_residual)
        added = extension["compressed"]
        for (name, region), m in extension["columns"].items():
            if m <= 0:
                continue
            art_key = "masked" if region == "masked" else "unmasked"
            grown[name] = bases[name] = extension["bases"][name]
            compressed[name] = {t: {**a, art_key: pad_c_high(a.get(art_key), m)} if isinstance(a, dict) else a
                                for t, a in compressed.get(name, {}).items()}
    else:
        added = project_all_parameters(models, masks or {}, bases, config, device=device, base_state_dict=base_sd)
    touched = {}
    for name, per_task in added.items():
        merged = dict(compressed.get(name, {}))
        merged.update(per_task)
        compressed[name] = touched[name] = merged
    diagnostics["task_weights"] = task_weights
    result = {"tasks": tasks, "added": new, "compressed": added}
    if extension is not None:
        result["captured_energy"] = diagnostics["captured_energy"] = dict(extension["captured_energy"])
        result["columns"] = diagnostics["columns"] = {f"{n} [{r}]": int(m) for (n, r), m in
                                                      extension["columns"].items()}
    out = output_dir or artifact_dir
    if os.path.realpath(out) == os.path.realpath(artifact_dir):
        for name, b in grown.items():
            save_basis(b, name, out)
        save_compressed_coefficients(touched, out)
        save_diagnostics(diagnostics, out)
    else:
        save_all_artifacts(bases, compressed, diagnostics, config, out)
    result["output_dir"] = out
    return result


def consolidated_config(config, energy_threshold=None, max_rank=None, low_bits=None, rtvq_stages=None, center=None):
    """The stored config with the arguments given put over it (None = as stored); the dataclass's own checks apply."""
    from dataclasses import replace
    over = {k: v for k, v in (("svd_energy_threshold", energy_threshold), ("svd_max_rank", max_rank),
                              ("svd_low_bits", low_bits), ("svd_rtvq_stages", rtvq_stages), ("svd_center", center))
            if v is not None}
    return replace(config, **over) if over else config


def consolidated_diagnostics(diagnostics: Dict[str, Any], kept, result: Dict[str, Any]) -> Dict[str, Any]:
    """diagnostics.json of a consolidated store: the stored one with ``task_weights`` restricted to the kept tasks and,
    when a task was dropped, renormalised (uniform where the store had none), and ``tasks`` / ``columns`` ({"param [region]": [r, r']}) /
    ``dropped_energy`` / ``noise_floor`` / ``promoted`` recorded; ``cluster_assignments`` and ``captured_energy`` lose
    the dropped tasks.  A pure function: the input is not touched."""
    out = dict(diagnostics)
    old = diagnostics.get("task_weights") or {}
    ws = {t: float(old[t]) for t in kept if t in old}
    tot = sum(ws.values())
    if len(ws) == len(kept) == len(old):      # no task left: the stored weights as they are
        out["task_weights"] = ws
    else:
        out["task_weights"] = ({t: ws[t] / tot for t in kept} if len(ws) == len(kept) and tot > 0
                               else {t: 1.0 / len(kept) for t in kept})
    out["tasks"] = list(kept)
    out["columns"] = {f"{n} [{r}]": [int(a), int(b)] for (n, r), (a, b) in result["columns"].items()}
    out["dropped_energy"] = {f"{n} [{r}]": float(v) for (n, r), v in result["dropped_energy"].items()}
    out["noise_floor"] = {f"{n} [{r}]": float(v) for (n, r), v in result.get("noise_floor", {}).items()}
    out["promoted"] = {f"{n} [{r}]": [int(a), int(b)] for (n, r), (a, b) in result.get("promoted", {}).items()}
    for key in ("cluster_assignments", "captured_energy"):      # other per-task records: the dropped tasks leave them too
        if isinstance(diagnostics.get(key), dict):
            out[key] = {t: v for t, v in diagnostics[key].items() if t in kept}
    return out


def _replace_store_files(staged: str, artifact_dir: str) -> None:
    """Move every file of the staged store over its counterpart in ``artifact_dir`` (os.replace, file by file: each file
    is old or new, never partial).  Files of the store that consolidation does not write (a merged model, masks) stay.
    The window: a failure INSIDE this loop -- after everything was computed and written to the staging directory --
    leaves a store that mixes old and new files; the staging directory is then kept, so that the move can be finished
    by hand."""
    for root, _, files in os.walk(staged):
        rel = os.path.relpath(root, staged)
        dst = artifact_dir if rel == "." else os.path.join(artifact_dir, rel)
        os.makedirs(dst, exist_ok=True)
        for f in files:
            os.replace(os.path.join(root, f), os.path.join(dst, f))


def consolidate_artifacts(artifact_dir: str, output_dir: str = None, tasks=None, energy_threshold=None, max_rank=None,
                          low_bits=None, rtvq_stages=None, center=None, min_sigma: float = 0.0, device: str = "cuda"
                          ) -> Dict[str, Any]:
    """Consolidate a stored artifact set: bases, rank, mean and coefficients re-derived from the artifacts alone
    (``compress.consolidate_bases``) -- after ``add_tasks_to_artifacts(extend_basis=True)`` grew the store, to drop
    tasks from it (``tasks``: the ones to keep; None = all), or to take it to another ``energy_threshold`` /
    ``max_rank`` / ``low_bits`` / ``rtvq_stages`` / ``center`` (None = as stored).  No checkpoint is read.
    The consolidated store goes to ``output_dir``; None = in place, and then through a temporary directory beside the
    store: everything is computed and written there first, so a failure up to that point leaves the old store whole;
    the files are then moved over the old ones one by one (``_replace_store_files`` states that window).  The dropped
    tasks are in no file of the new store; ``tasks``, ``columns`` and ``dropped_energy`` are recorded in
    diagnostics.json.  A region whose c_low the quantizer cannot represent is stored on the high side and listed under
    ``promoted`` (``compress.consolidate_bases``): no store with non-finite coefficients is written.
    Returns {"tasks", "dropped", "columns", "dropped_energy", "promoted", "skipped", "output_dir"}."""
    import shutil
    import tempfile
    from .compress import consolidate_bases, consolidate_task_list, check_consolidate_room
    art = load_all_artifacts(artifact_dir, device="cpu")
    diagnostics, bases, compressed = art["diagnostics"], art["bases"], art["compressed"]
    kept = consolidate_task_list(compressed, tasks)
    check_consolidate_room(bases)
    config = consolidated_config(art["config"], energy_threshold, max_rank, low_bits, rtvq_stages, center)
    stored = _stored_tasks(compressed, diagnostics)
    res = consolidate_bases(compressed, bases, config, tasks=kept, min_sigma=min_sigma, device=device)
    new_comp = {n: ({t: a for t, a in per_task.items() if t in kept} if n in res["skipped"] else per_task)
                for n, per_task in res["compressed"].items()}
    new_diag = consolidated_diagnostics(diagnostics, kept, res)
    in_place = output_dir is None or os.path.realpath(output_dir) == os.path.realpath(artifact_dir)
    out = artifact_dir if in_place else output_dir
    if in_place:
        parent = os.path.dirname(os.path.realpath(artifact_dir))
        staged = tempfile.mkdtemp(prefix=".consolidate-", dir=parent)
        try:
            save_all_artifacts(res["bases"], new_comp, new_diag, config, staged)
        except BaseException:
            shutil.rmtree(staged, ignore_errors=True)      # nothing of the store was touched
            raise
        _replace_store_files(staged, artifact_dir)
        shutil.rmtree(staged, ignore_errors=True)
    else:
        save_all_artifacts(res["bases"], new_comp, new_diag, config, out)
    return {"tasks": kept, "dropped": [t for t in stored if t not in kept],
            "columns": new_diag["columns"], "dropped_energy": new_diag["dropped_energy"],
            "promoted": new_diag["promoted"], "skipped": res["skipped"],
            "output_dir": out}


def remerge_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None, weighting: Optional[str] = None,
                           cluster_k: Optional[int] = None, performance_file: Optional[str] = None,
                           temperature: Optional[float] = None, device: str = "cuda", update_store: bool = False
                           ) -> Dict[str, Any]:
    """Merge a stored artifact set again under another weighting -- the reference's Steps 6 and 7 (compute_weights
    weighting.py:266-329, cluster_tasks clustering.py:198-245, merge_all_parameters / merge_with_clustering merge.py:304-626)
    on a store, without the fine-tuned checkpoints.  load_all_artifacts -> adopt_artifacts -> weights -> merge ->
    apply_merged_deltas.  Masks are not stored (reload.py:204-205): exact for unmasked runs, as ``reconstruct_from_artifacts``.

    ``weighting``: None = the stored ``diagnostics["task_weights"]`` -- then this is ``reconstruct_from_artifacts`` bit
    for bit; "uniform" / "performance" = ``compute_weights`` over the stored tasks (``performance_file``;
    ``temperature`` None = the stored config's svd_weighting_temperature); "cluster" = the tasks are clustered on the
    Gram of what the store reconstructs (``cluster_tasks_from_artifacts``, k-means, ``cluster_k`` None = the stored
    config's svd_cluster_k), the weights are ``compute_weights(..., cluster_assignments=)`` and the merge is
    ``merge_with_clustering``.  ``base_model_path``: a path or a state dict.

    Returns {"merged_state_dict", "weights", "cluster_assignments" (None unless "cluster"), "diagnostics", "config"}.
    The store's files are left alone unless ``update_store``: then diagnostics.json is rewritten with the weights used
    (``task_weights``) and the labels (``cluster_assignments``; dropped when the weighting is not "cluster"), and
    clusters.json is written (or removed) beside it.  Nothing else of the store is touched."""
    from .clustering import cluster_tasks_from_artifacts
    from .driver import adopt_artifacts
    from .merge import apply_merged_deltas, merge_all_parameters, merge_with_clustering
    from .weighting import compute_weights
    if weighting not in (None, "uniform", "performance", "cluster"):
        raise ValueError(f"Unknown weighting strategy: {weighting}")
    art = load_all_artifacts(artifact_dir, device=device)
    config, diagnostics = art["config"], art["diagnostics"]
    stored = _stored_tasks(art["compressed"], diagnostics)
    bases, compressed = adopt_artifacts(art.pop("bases"), art.pop("compressed"), config, device=device)
    shapes = {n: torch.Size(d["original_shape"]) for n, d in diagnostics.get("per_parameter", {}).items()
              if d.get("original_shape") is not None}
    assignments = None
    if weighting is None:      # reconstruct_from_artifacts' own lines
        tasks = list(diagnostics.get("task_weights", {}).keys())
        if not tasks:
            tasks = list(next(iter(compressed.values())).keys())
        weights = diagnostics.get("task_weights") or {t: 1.0 / len(tasks) for t in tasks}
    else:
        if not stored:
            raise ValueError(f"{artifact_dir} holds no task")
        T = float(config.svd_weighting_temperature if temperature is None else temperature)
        if weighting == "cluster":
            k = int(config.svd_cluster_k if cluster_k is None else cluster_k)
            assignments = cluster_tasks_from_artifacts(compressed, bases, k, method="kmeans", device=device)
        weights = compute_weights(stored, weighting_strategy=weighting, performance_file=performance_file, temperature=T,
                                  cluster_assignments=assignments)
    if assignments is not None:
        merged = merge_with_clustering(compressed, bases, {}, weights, assignments, shapes, config, device=device)
    else:
        merged = merge_all_parameters(compressed, bases, {}, weights, shapes, config, device=device, verbose=False)
    base = _load_base(base_model_path, device)
    out = apply_merged_deltas(base, merged, device=device, verbose=False)
    if output_path:
        torch.save(out, output_path)
    if update_store:
        diagnostics["task_weights"] = {t: float(w) for t, w in weights.items()}
        clusters = os.path.join(artifact_dir, "clusters.json")
        if assignments is not None:
            diagnostics["cluster_assignments"] = {t: int(c) for t, c in assignments.items()}
            with open(clusters, "w") as f:
                json.dump(diagnostics["cluster_assignments"], f, indent=2)
        else:
            diagnostics.pop("cluster_assignments", None)
            if os.path.exists(clusters):
                os.remove(clusters)
        save_diagnostics(diagnostics, artifact_dir)
    return {"merged_state_dict": out, "weights": weights, "cluster_assignments": assignments,
            "diagnostics": diagnostics, "config": config}


_NO_BASE = object()


def _adopted_store(artifact_dir: str, tasks, device, base_model_path=_NO_BASE):
    """The front of the ``*_from_artifacts`` merges over every task's own values: load_all_artifacts -> the ValueError
    for a name of ``tasks`` that the store lacks -> the base (``_load_base``; none without ``base_model_path``) ->
    adopt_artifacts.  Returns (config, diagnostics, bases, compressed, shapes, base or None, the base's tensors that the
    store covers or None)."""
    from .driver import adopt_artifacts
    art = load_all_artifacts(artifact_dir, device=device)
    config, diagnostics = art["config"], art["diagnostics"]
    if tasks is not None:
        known = {t for per_task in art["compressed"].values() for t in per_task}
        for t in tasks:
            if t not in known:
                raise ValueError(f"unknown task {t!r}: the artifacts hold {sorted(known)}")
    base = None if base_model_path is _NO_BASE else _load_base(base_model_path, device)
    bases, compressed = adopt_artifacts(art.pop("bases"), art.pop("compressed"), config, device=device)
    shapes = {n: torch.Size(d["original_shape"]) for n, d in diagnostics.get("per_parameter", {}).items()
              if d.get("original_shape") is not None}
    covered = None if base is None else {n: b for n, b in base.items() if n in compressed}
    return config, diagnostics, bases, compressed, shapes, base, covered


def _merged_over_base(merged: Dict[str, torch.Tensor], base: Dict[str, torch.Tensor], output_path
                      ) -> Dict[str, torch.Tensor]:
    """The back of the same: the merged tensors, the base's other tensors cloned (as apply_merged_deltas does), saved on
    the CPU when a path is given."""
    out = {n: (merged[n] if n in merged else b.clone()) for n, b in base.items()}
    if output_path:
        torch.save({n: v.cpu() for n, v in out.items()}, output_path)
    return out


def ties_merge_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None, density: float = 0.2,
                              scaling: float = 1.0, merge_func: str = "mean", tasks=None, device: str = "cuda"
                              ) -> Dict[str, Any]:
    """The sign-elected (TIES) merge of a stored artifact set (``merge.ties_merge_parameters``, which see for the
    definition): load_all_artifacts -> adopt_artifacts -> ties_merge_parameters with the base inside the launch -> the
    base's other tensors cloned (as apply_merged_deltas does) -> optional save.  Masks are not stored (reload.py:204-205):
    a masked run's store is refused with a ValueError naming the parameter.  ``base_model_path``: a path or a state dict;
    ``tasks``: names (None = every stored task).  The store's files are only read.

    Returns {"merged_state_dict", "stats" (thresholds, kept counts, row counters, rows), "diagnostics", "config"}."""
    from .merge import ties_merge_parameters
    if not (isinstance(density, (int, float)) and 0.0 < float(density) <= 1.0):      # before any file or device work
        raise ValueError(f"density must be in (0, 1], got {density!r}")
    config, diagnostics, bases, compressed, shapes, base, covered = _adopted_store(artifact_dir, tasks, device,
                                                                                   base_model_path)
    merged, stats = ties_merge_parameters(compressed, bases, shapes, config, density=density, scaling=scaling,
                                          merge_func=merge_func, tasks=tasks, base_state_dict=covered, device=device,
                                          return_stats=True)
    out = _merged_over_base(merged, base, output_path)
    return {"merged_state_dict": out, "stats": stats, "diagnostics": diagnostics, "config": config}


def breadcrumbs_merge_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None, density: float = 0.9,
                                     gamma: float = 0.01, scaling: float = 1.0, sign_election: bool = False,
                                     merge_func: str = "sum", tasks=None, device: str = "cuda") -> Dict[str, Any]:
    """The Model Breadcrumbs merge of a stored artifact set, the per-tensor TIES trim with ``gamma=0,
    sign_election=True, merge_func="mean"`` (``merge.breadcrumbs_merge_parameters``, which see for the definition):
    load_all_artifacts -> adopt_artifacts -> breadcrumbs_merge_parameters with the base inside the launch -> the base's
    other tensors cloned (as apply_merged_deltas does) -> optional save.  Masks are not stored (reload.py:204-205): a
    masked run's store is refused with a ValueError naming the parameter.  ``base_model_path``: a path or a state dict;
    ``tasks``: names (None = every stored task).  The store's files are only read.

    Returns {"merged_state_dict", "stats" (bands and kept counts per parameter and task, row counters, rows),
    "diagnostics", "config"}."""
    from .merge import _crumbs_arguments, breadcrumbs_merge_parameters
    _crumbs_arguments(density, gamma, scaling, merge_func)      # before any file or device work
    config, diagnostics, bases, compressed, shapes, base, covered = _adopted_store(artifact_dir, tasks, device,
                                                                                   base_model_path)
    merged, stats = breadcrumbs_merge_parameters(compressed, bases, shapes, config, density=density, gamma=gamma,
                                                 scaling=scaling, sign_election=sign_election, merge_func=merge_func,
                                                 tasks=tasks, base_state_dict=covered, device=device, return_stats=True)
    out = _merged_over_base(merged, base, output_path)
    return {"merged_state_dict": out, "stats": stats, "diagnostics": diagnostics, "config": config}


def dare_merge_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None, drop_rate: float = 0.9,
                              seed: int = 0, rescale: bool = True, weights=None, normalize: bool = False,
                              scaling: float = 1.0, tasks=None, device: str = "cuda") -> Dict[str, Any]:
    """The drop-and-rescale (DARE) merge of a stored artifact set, task arithmetic with ``drop_rate=0``
    (``merge.dare_merge_parameters``, which see for the definition): load_all_artifacts -> adopt_artifacts ->
    dare_merge_parameters with the base inside the launch -> the base's other tensors cloned (as apply_merged_deltas
    does) -> optional save.  Masks are not stored (reload.py:204-205): a masked run's store is refused with a ValueError
    naming the parameter.  ``base_model_path``: a path or a state dict; ``tasks``: names (None = every stored task).  The
    store's files are only read.

    Returns {"merged_state_dict", "stats" (kept counts, rows, drop threshold), "diagnostics", "config"}."""
    from .merge import _dare_arguments, dare_merge_parameters
    _dare_arguments(drop_rate, seed)      # before any file or device work
    config, diagnostics, bases, compressed, shapes, base, covered = _adopted_store(artifact_dir, tasks, device,
                                                                                   base_model_path)
    merged, stats = dare_merge_parameters(compressed, bases, shapes, config, drop_rate=drop_rate, seed=seed,
                                          rescale=rescale, weights=weights, normalize=normalize, scaling=scaling,
                                          tasks=tasks, base_state_dict=covered, device=device, return_stats=True)
    out = _merged_over_base(merged, base, output_path)
    return {"merged_state_dict": out, "stats": stats, "diagnostics": diagnostics, "config": config}


def consensus_merge_from_artifacts(artifact_dir: str, base_model_path, output_path: str = None,
                                   mask_output_path: str = None, tall_lambda=0.4, k: int = 2, scaling: float = 1.0,
                                   tasks=None, remove_keys=None, device: str = "cuda") -> Dict[str, Any]:
    """TALL masks and the consensus merge of a stored artifact set (``merge.consensus_merge_parameters``, which see for
    the definition): load_all_artifacts -> adopt_artifacts -> one launch per plan with the base inside it -> the base's
    other tensors cloned (as apply_merged_deltas does) -> optional save.  ``mask_output_path`` receives
    ``numpy.savez(path, **{task: packed mask})`` over the sorted keys of the base minus ``remove_keys`` -- named
    TALL_mask_{T}task.npz it is what ``load_tall_mask_file``, ``combine_tall_masks_packed`` and ``--mask-dir`` read, with
    the base as the reference state dict.  Masks are not stored (reload.py:204-205): a masked run's store is refused with
    a ValueError naming the parameter.  ``base_model_path``: a path or a state dict; ``tasks``: names (None = every
    stored task).  The store's files are only read.

    Returns {"merged_state_dict", "masks" ({task: packed uint8 tensor} or None), "stats" (active, agreement, rows),
    "diagnostics", "config"}."""
    import numpy as np
    from .merge import _tall_arguments, consensus_merge_parameters
    who = "consensus_merge_parameters"
    if not hasattr(tall_lambda, "get"):
        _tall_arguments(who, tall_lambda, None, [None], check_k=False)      # one number for every task: before any file or device work
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"{who}: k must be an integer in [0, merged tasks], got {k!r}")
    config, diagnostics, bases, compressed, shapes, base, covered = _adopted_store(artifact_dir, tasks, device,
                                                                                   base_model_path)
    want_masks = mask_output_path is not None
    got = consensus_merge_parameters(compressed, bases, shapes, config, tall_lambda=tall_lambda, k=k, scaling=scaling,
                                     tasks=tasks, base_state_dict=covered,
                                     reference_state_dict=base if want_masks else None, remove_keys=remove_keys,
                                     return_masks=want_masks, device=device, return_stats=True)
    merged, masks, stats = got if want_masks else (got[0], None, got[1])
    out = _merged_over_base(merged, base, output_path)
    if want_masks:
        with open(mask_output_path, "wb") as f:      # a file object: numpy appends no suffix to the caller's name
            np.savez(f, **{t: m.cpu().numpy() for t, m in masks.items()})
    return {"merged_state_dict": out, "masks": masks, "stats": stats, "diagnostics": diagnostics, "config": config}


EMR_UNIFIED_FILE, EMR_RESCALER_FILE = "emr_unified.pt", "emr_rescalers.json"


def save_emr_merge(output_dir: str, unified: Dict[str, torch.Tensor], masks: Dict[str, torch.Tensor],
                   rescalers: Dict[str, float], stats: Optional[Dict[str, Any]] = None) -> Dict[str, str]:
    """The three files of an EMR merge (``merge.emr_merge_parameters``): emr_unified.pt ({param: fp32 tensor}),
    EMR_mask_{T}task.npz (``numpy.savez(file, **{task: packed mask})``, the container of a TALL_mask_{T}task.npz:
    ``load_tall_mask_file`` reads it back, with the unified tensors as the reference state dict) and emr_rescalers.json
    ({"tasks", "rescalers", "mask_file"} and the statistics when given; Python writes a float so that it reads back
    exactly).  Returns {"unified", "masks", "rescalers"}: the paths."""
    import numpy as np
    os.makedirs(output_dir, exist_ok=True)
    tasks = sorted(masks)
    paths = {"unified": os.path.join(output_dir, EMR_UNIFIED_FILE),
             "masks": os.path.join(output_dir, f"EMR_mask_{len(tasks)}task.npz"),
             "rescalers": os.path.join(output_dir, EMR_RESCALER_FILE)}
    torch.save({n: v.detach().cpu() for n, v in unified.items()}, paths["unified"])
    with open(paths["masks"], "wb") as f:      # a file object: numpy appends no suffix to the name
        np.savez(f, **{t: masks[t].detach().cpu().numpy() for t in tasks})
    record = {"tasks": tasks, "rescalers": {t: float(rescalers[t]) for t in tasks},
              "mask_file": os.path.basename(paths["masks"])}
    if stats is not None:
        record.update({"abs_sum": {t: float(stats["abs_sum"][t]) for t in tasks},
                       "masked_sum": {t: float(stats["masked_sum"][t]) for t in tasks},
                       "active": {t: int(stats["active"][t]) for t in tasks}, "rows": int(stats["rows"])})
    with open(paths["rescalers"], "w") as f:
        json.dump(record, f, indent=2)
    return paths


def load_emr_merge(output_dir: str, device: str = "cpu"):
    """(unified, masks {task: packed uint8 tensor}, rescalers, record) from the files ``save_emr_merge`` wrote; both
    loaders execute nothing from the files."""
    import numpy as np
    with open(os.path.join(output_dir, EMR_RESCALER_FILE)) as f:
        record = json.load(f)
    unified = torch.load(os.path.join(output_dir, EMR_UNIFIED_FILE), map_location=device, weights_only=True)
    with np.load(os.path.join(output_dir, record["mask_file"]), allow_pickle=False) as z:
        masks = {t: torch.from_numpy(np.ascontiguousarray(z[t])).reshape(-1) for t in z.files}
    return unified, masks, {t: float(x) for t, x in record["rescalers"].items()}, record


def emr_from_artifacts(artifact_dir: str, output_dir: str, tasks=None, device: str = "cuda") -> Dict[str, Any]:
    """The EMR merge of a stored artifact set (``merge.emr_merge_parameters``, which see for the definition):
    load_all_artifacts -> adopt_artifacts -> one launch per plan -> ``save_emr_merge`` into ``output_dir``.  The mask
    streams run over the store's own parameters in sorted order.  Masks are not stored (reload.py:204-205): a masked
    run's store is refused with a ValueError naming the parameter.  ``tasks``: names (None = every stored task).  The
    store's files are only read.

    Returns {"unified", "masks", "rescalers", "stats" (abs_sum, masked_sum, active, rows), "paths", "diagnostics",
    "config"}."""
    from .merge import emr_merge_parameters
    config, diagnostics, bases, compressed, shapes, _, _ = _adopted_store(artifact_dir, tasks, device)
    unified, masks, rescalers, stats = emr_merge_parameters(compressed, bases, shapes, config, tasks=tasks,
                                                            device=device, return_stats=True)
    paths = save_emr_merge(output_dir, unified, masks, rescalers, stats)
    return {"unified": unified, "masks": masks, "rescalers": rescalers, "stats": stats, "paths": paths,
            "diagnostics": diagnostics, "config": config}


def emr_task_model_from_files(output_dir: str, task: str, base_model_path, output_path: str = None, rescale=None,
                              device: str = "cuda") -> Dict[str, Any]:
    """Task ``task``'s model from the files of ``emr_from_artifacts`` and a base model: ``load_emr_merge`` -> one launch
    (``merge.emr_task_state_dict``, the base inside it) -> the base's other tensors cloned (as apply_merged_deltas does)
    -> optional save.  ``base_model_path``: a path or a state dict; ``rescale`` overrides the stored scalar.

    Returns {"state_dict", "rescaler"}."""
    from .merge import emr_task_state_dict
    unified, masks, rescalers, _ = load_emr_merge(output_dir, device="cpu")
    if task not in masks or task not in rescalers:
        raise ValueError(f"unknown task {task!r}: {output_dir} holds {sorted(masks)}")
    base = _load_base(base_model_path, device)
    covered = {n: b for n, b in base.items() if n in unified}
    got = emr_task_state_dict(unified, masks, rescalers, task, base_state_dict=covered, rescale=rescale, device=device)
    out = {n: (got[n] if n in got else b.clone()) for n, b in base.items()}
    if output_path:
        torch.save({n: v.cpu() for n, v in out.items()}, output_path)
    return {"state_dict": out, "rescaler": float(rescalers[task] if rescale is None else rescale)}


def reload_merged_model_from_artifacts(artifact_dir: str, device: str = "cpu") -> Dict[str, torch.Tensor]:
    """Reference reload.py:60-139: a pre-saved merged_state_dict.pt in the artifact directory wins; otherwise the
    merged model is rebuilt from bases + coefficients + the base model named in the stored config."""
    pre = os.path.join(artifact_dir, "merged_state_dict.pt")
    if os.path.exists(pre):
        print(f"Loading pre-saved merged model from {pre}")
        return torch.load(pre, map_location=device, weights_only=True)
    print("No pre-saved merged model found, reconstructing from artifacts...")
    config = load_config(artifact_dir)
    base_path = getattr(config, "base_model_path", "") if not isinstance(config, dict) else config.get("base_model_path", "")
    if not base_path or not os.path.exists(base_path):
        raise FileNotFoundError(f"Base model path not found in config or doesn't exist: {base_path}. Please provide "
                                "base model path in artifacts config or use reconstruct_from_artifacts instead.")
    return reconstruct_from_artifacts(artifact_dir, base_path, None, device=device)["merged_state_dict"]
