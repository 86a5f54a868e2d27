"""
Task-vector compression with the reference's call signatures and return layouts
(reference src/svd_hybrid/compress.py:6-207).

``project_all_parameters`` is the batched form of the second route below: stored bases go into plans
(``driver.adopt_bases``) and ONE ``svdq_plan_project`` per plan projects and quantizes every new task.  It is a name of its
own because its last bits differ from ``svdq_project``'s grid-stride sums.

Two routes produce identical artifact dicts:
  * bases that came out of ``driver.run_basis_and_compress`` / ``driver.build_bases`` carry the
    coefficients the fused pass 2 already computed; ``compress_all_parameters`` just assembles them;
  * any other basis (a caller's own U) goes through ``svdq_project`` + the GPU quantizer, one
    (parameter, task) at a time, exactly like the reference's loops.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _native as nat
from .pipeline import prepare_vector, resolve_device, _ptr, _stream_ptr
from .rtvq import RTVQQuantizer


def project_to_basis(delta: torch.Tensor, U_high: torch.Tensor, U_low: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference compress.py:6-21: (U_high.float().T @ delta, U_low.float().T @ delta)."""
    return _project(delta, U_high, U_low, None)


def _project(delta, U_high, U_low, mean):
    lib = nat.lib()
    dev = resolve_device(U_high.device if U_high.is_cuda else (delta.device if delta.is_cuda else "cuda"))
    out_dev = delta.device
    x = prepare_vector(delta, dev)
    D = x.numel()
    k = U_high.shape[1] if U_high.dim() == 2 else 0
    nl = U_low.shape[1] if U_low.dim() == 2 else 0
    if k + nl == 0:
        return torch.zeros(0, device=out_dev), torch.zeros(0, device=out_dev)
    if (k and U_high.shape[0] != D) or (nl and U_low.shape[0] != D):
        raise ValueError(f"Shape mismatch: basis rows vs delta length {D}")
    fp16 = (U_high.dtype == torch.float16) if k else (U_low.dtype == torch.float16)
    dt = torch.float16 if fp16 else torch.float32
    uh = U_high.to(device=dev, dtype=dt).contiguous() if k else None
    ul = U_low.to(device=dev, dtype=dt).contiguous() if nl else None
    m = prepare_vector(mean.squeeze() if mean.dim() > 1 else mean, dev) if mean is not None else None
    if k + nl <= 32:
        c = _project_cols(lib, dev, uh, ul, fp16, D, k, nl, x, m)
    else:
        # the kernel takes up to 32 columns (the path never has more than N <= 32); a caller's own wider basis
        # (the reference's tests project onto full square bases) goes through in column groups
        parts = []
        for u, n in ((uh, k), (ul, nl)):
            for c0 in range(0, n, 32):
                cn = min(32, n - c0)
                parts.append(_project_cols(lib, dev, u[:, c0:c0 + cn].contiguous(), None, fp16, D, cn, 0, x, m))
        c = torch.cat(parts)
    c = c.to(out_dev)
    return c[:k], c[k:]


def _project_cols(lib, dev, uh, ul, fp16, D, k, nl, x, m):
    c = torch.empty(k + nl, dtype=torch.float32, device=dev)
    work = torch.empty(int(lib.svdq_project_work_bytes(D, k + nl)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.svdq_project(_ptr(uh), _ptr(ul), int(fp16), D, k, nl, _ptr(x), _ptr(m), _ptr(c), _ptr(work),
                                   _stream_ptr()), "svdq_project")
    return c


def compress_single_task(task_delta: torch.Tensor, U_high: torch.Tensor, U_low: torch.Tensor,
                         quantizer: RTVQQuantizer, device: str = "cpu", mean: Optional[torch.Tensor] = None) -> Dict:
    """Reference compress.py:24-56."""
    c_high, c_low = _project(task_delta, U_high, U_low, mean)
    c_high_fp16 = c_high.half() if c_high.dtype != torch.float16 else c_high
    return {"c_high_fp16": c_high_fp16.cpu(), "c_low_quant": quantizer.quantize(c_low.cpu())}


def compress_masked_regions(task_deltas_masked: Dict[str, torch.Tensor],
                            task_deltas_unmasked: Optional[Dict[str, torch.Tensor]], basis_masked: Dict,
                            basis_unmasked: Optional[Dict], quantizer: RTVQQuantizer, device: str = "cpu"
                            ) -> Dict[str, Dict]:
    """Reference compress.py:59-111."""
    out = {}
    mean_m = basis_masked.get("mean") if basis_masked is not None else None
    mean_u = basis_unmasked.get("mean") if basis_unmasked is not None else None
    for task, dm in task_deltas_masked.items():
        art = {}
        if basis_masked is not None and len(dm) > 0:
            art["masked"] = compress_single_task(dm, basis_masked["U_high"], basis_masked["U_low"], quantizer, device,
                                                 mean=mean_m)
        else:
            art["masked"] = None
        if (basis_unmasked is not None and task_deltas_unmasked is not None and task in task_deltas_unmasked
                and len(task_deltas_unmasked[task]) > 0):
            art["unmasked"] = compress_single_task(task_deltas_unmasked[task], basis_unmasked["U_high"],
                                                   basis_unmasked["U_low"], quantizer, device, mean=mean_u)
        else:
            art["unmasked"] = None
        out[task] = art
    return out


def compress_parameter(param_name: str, task_vectors: Dict[str, Dict[str, torch.Tensor]],
                       mask: Optional[torch.Tensor], basis: Dict, quantizer: RTVQQuantizer,
                       include_noise: bool = False, min_mask_size: int = 10, device: str = "cpu") -> Optional[Dict]:
    """Reference compress.py:114-170."""
    from .mask_loader import apply_mask_to_tensor, get_unmasked_portion
    deltas = {t: tv[param_name] for t, tv in task_vectors.items() if param_name in tv}
    if not deltas:
        return None
    masked, unmasked = {}, {}
    for t, d in deltas.items():
        if mask is not None and mask.shape == d.shape:
            if mask.sum() >= min_mask_size:
                masked[t] = apply_mask_to_tensor(d, mask)
            else:
                masked[t] = torch.tensor([])
            if include_noise:
                unmasked[t] = get_unmasked_portion(d, mask)
        else:
            masked[t] = d.flatten()
    return compress_masked_regions(masked, unmasked if include_noise else None, basis.get("masked"),
                                   basis.get("noise") if include_noise else None, quantizer, device)


def compress_all_parameters(task_vectors: Dict[str, Dict[str, torch.Tensor]], masks: Dict[str, torch.Tensor],
                            bases: Dict[str, Dict], config, device: str = "cpu") -> Dict[str, Dict]:
    """Reference compress.py:173-207.  Parameters in sorted order, tasks in insertion order, one
    quantizer (b, S) for the whole run."""
    import gc
    from .driver import artifacts_from_batch
    quantizer = RTVQQuantizer(num_bits=config.svd_low_bits, num_stages=config.svd_rtvq_stages)
    out = {}
    # assembling ~10^4 small dictionaries and tensors: keep the cyclic collector from re-walking them all
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        for name in sorted(bases.keys()):
            basis = bases[name]
            fused = artifacts_from_batch(name, basis, task_vectors, config)
            if fused is not None:
                out[name] = fused
                continue
            comp = compress_parameter(name, task_vectors, masks.get(name), basis, quantizer,
                                      include_noise=config.svd_include_noise,
                                      min_mask_size=config.svd_min_mask_size, device=device)
            if comp is not None:
                out[name] = comp
    finally:
        if gc_was_on:
            gc.enable()
    return out


def project_all_parameters(task_vectors: Dict[str, Dict[str, torch.Tensor]], masks: Optional[Dict[str, torch.Tensor]],
                           bases: Dict[str, Dict], config, device: str = "cuda",
                           base_state_dict: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, Dict]:
    """``compress_all_parameters`` for NEW tasks against bases that already exist -- loaded from disk, adopted, a
    caller's own U -- in one ``svdq_plan_project`` per plan instead of a selection, a projection launch pair, a
    device-to-host copy and a quantizer call per (parameter, region, task).  Returns exactly the dictionary layout
    ``compress_all_parameters`` returns: {param: {task: {"masked": {...}, "unmasked": ... | None}}}, CPU tensors.

    ``task_vectors``: {task: {param: tensor}}, up to 32 tasks; with ``base_state_dict`` they hold FINE-TUNED weights and
    finetuned - base is formed inside the launch (no task vectors in memory).  Tensors that are all fp16 or all bf16
    (base included) are read as they are.  A masked parameter (``masks[name]`` of the tensor's shape) is read through
    index lists built once per parameter (svdq_maskset_indices); its noise region, when ``config.svd_include_noise``,
    through the inverted list against ``bases[name]["noise"]``.  A selected count that differs from the stored D raises a
    ``ValueError`` naming the parameter.  What ``adopt_bases`` declines -- and a parameter whose mask selects fewer than
    ``svd_min_mask_size`` elements -- goes through ``compress_parameter``, unchanged (there ``task_vectors`` must hold
    task vectors: with ``base_state_dict`` the difference is formed first, for those parameters only)."""
    import gc
    from . import mask_loader as ml
    from .driver import adopt_bases
    from .pipeline import native_input_dtype, prepare_input, task_artifact
    masks = masks or {}
    tasks = list(task_vectors.keys())
    if not tasks:
        return {}
    if len(tasks) > nat.MAX_TASKS:
        raise ValueError(f"project_all_parameters takes at most {nat.MAX_TASKS} tasks per call, got {len(tasks)}")
    dev = resolve_device(device)
    include_noise = bool(config.svd_include_noise)

    def usable_mask(name):
        """The mask as compress_parameter applies it: only when its shape is the tensors' shape."""
        m = masks.get(name)
        if m is None:
            return None
        shapes = {tuple(tv[name].shape) for tv in task_vectors.values() if name in tv}
        return m if shapes == {tuple(m.shape)} else None

    names = [n for n in sorted(bases.keys()) if any(n in tv for tv in task_vectors.values())]
    mask_of = {n: usable_mask(n) for n in names}
    # masks that select fewer than min_mask_size elements empty the masked region (compress.py:143-147): per parameter
    small_mask = {n for n, m in mask_of.items() if m is not None and int(m.sum()) < config.svd_min_mask_size}
    batched_bases = {n: bases[n] for n in names if n not in small_mask}
    covered = [t[n] for t in task_vectors.values() for n in batched_bases if n in t]
    if base_state_dict is not None:
        missing = [n for n in names if n not in base_state_dict]
        if missing:
            raise ValueError(f"base_state_dict lacks parameter {missing[0]!r}")
        covered += [base_state_dict[n] for n in batched_bases]
    in_dtype = native_input_dtype(covered)
    batches, declined = adopt_bases(batched_bases, config, len(tasks), device=dev, input_dtype=in_dtype)

    out: Dict[str, Dict] = {}
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.device(dev):
            for batch in batches:
                plan = batch.plan
                P, N = plan.P, plan.N
                stored = [int(r) for r in batch.small.rows]
                # index lists, once per masked parameter of the plan
                mnames = []
                for name, _ in batch.entries:
                    if mask_of[name] is not None and name not in mnames:
                        mnames.append(name)
                idx_true = idx_false = {}
                ms = None
                if mnames:
                    ms = ml.MaskSet([int(mask_of[n].numel()) for n in mnames], dev)
                    it, if_, ct, cf = ms.indices([mask_of[n] for n in mnames], include_noise)
                    counts = torch.stack([ct, cf if cf is not None else torch.zeros_like(ct)]).cpu().tolist()
                    idx_true = {n: (it[q], counts[0][q]) for q, n in enumerate(mnames)}
                    idx_false = {n: (if_[q], counts[1][q]) for q, n in enumerate(mnames)} if include_noise else {}
                keep, tab, btab, itab, active = [], [0] * (P * N), [0] * P, [0] * P, [False] * P
                for i, (name, region) in enumerate(batch.entries):
                    if region == "noise" and not include_noise:
                        continue      # compress_parameter hands no noise basis on: "unmasked" stays None
                    m = mask_of[name]
                    if region == "noise" and m is None:
                        continue      # no mask, no noise region (compress.py:150-152)
                    numel = None
                    for t, task in enumerate(tasks):
                        x = task_vectors[task].get(name)
                        if x is None:
                            continue
                        v = prepare_input(x, dev, in_dtype)
                        numel = v.numel()
                        keep.append(v)
                        tab[i * N + t] = v.data_ptr()
                    if m is not None:
                        lst, count = (idx_false if region == "noise" else idx_true)[name]
                        keep.append(lst)
                        itab[i] = lst.data_ptr()
                    else:
                        count = numel
                    if count != stored[i]:
                        raise ValueError(f"parameter {name!r} [{region}]: {count} selected elements, the stored basis "
                                         f"has D = {stored[i]}")
                    if base_state_dict is not None:
                        b = prepare_input(base_state_dict[name], dev, in_dtype)
                        if b.numel() != numel:
                            raise ValueError(f"parameter {name!r}: the base tensor has {b.numel()} elements, the "
                                             f"task tensors {numel}")
                        keep.append(b)
                        btab[i] = b.data_ptr()
                    active[i] = True
                has_idx = any(itab)
                if has_idx:
                    # a plan mixes masked and unmasked entries: an unmasked one reads through the identity list
                    for i, (name, region) in enumerate(batch.entries):
                        if active[i] and not itab[i]:
                            ident = torch.arange(stored[i], dtype=torch.int32, device=dev)
                            keep.append(ident)
                            itab[i] = ident.data_ptr()
                rows_dev = torch.tensor([stored[i] if active[i] else 0 for i in range(P)], dtype=torch.int64).to(dev)
                table = torch.tensor(tab, dtype=torch.int64).to(dev)
                base_table = torch.tensor(btab, dtype=torch.int64).to(dev) if base_state_dict is not None else None
                index_table = torch.tensor(itab, dtype=torch.int64).to(dev) if has_idx else None
                sm = plan.project_tasks(table, base_table=base_table, index_table=index_table, rows_dev=rows_dev)
                del keep, ms
                for i, (name, region) in enumerate(batch.entries):
                    art_key = "masked" if region == "masked" else "unmasked"
                    per_task = out.setdefault(name, {})
                    for t, task in enumerate(tasks):
                        if name not in task_vectors[task]:
                            continue
                        art = per_task.setdefault(task, {"masked": None, "unmasked": None})
                        if active[i]:
                            art[art_key] = task_artifact(plan, sm, i, t)
        # the per-parameter route for whatever did not go into a plan
        rest = [n for n in names if n not in out]
        if rest:
            quantizer = RTVQQuantizer(num_bits=config.svd_low_bits, num_stages=config.svd_rtvq_stages)
            for name in rest:
                tv = task_vectors
                if base_state_dict is not None:
                    b = base_state_dict[name]
                    tv = {t: {name: (v[name].to(dev).float() - b.to(dev).float())} for t, v in task_vectors.items()
                          if name in v}
                comp = compress_parameter(name, tv, masks.get(name), bases[name], quantizer,
                                          include_noise=include_noise, min_mask_size=config.svd_min_mask_size,
                                          device=device)
                if comp is not None:
                    out[name] = comp
    finally:
        if gc_was_on:
            gc.enable()
    return {n: out[n] for n in sorted(out)}
