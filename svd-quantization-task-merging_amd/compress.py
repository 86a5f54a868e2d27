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
    # fp16 kernels only when every array that has columns is fp16; a mix is lifted to fp32, never rounded down
    fp16 = k + nl > 0 and all(u.dtype == torch.float16 for u, n in ((U_high, k), (U_low, nl)) if n)
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


def _projection_setup(task_vectors, masks, bases, config, device, base_state_dict, who: str):
    """What ``project_all_parameters`` and ``extend_bases`` decide before any plan runs: the task order, the parameters
    the new tasks hold, which masks apply, the input dtype, and the adoption of the bases into plans."""
    from .driver import adopt_bases
    from .pipeline import native_input_dtype
    masks = masks or {}
    tasks = list(task_vectors.keys())
    if len(tasks) > nat.MAX_TASKS:
        raise ValueError(f"{who} takes at most {nat.MAX_TASKS} tasks per call, got {len(tasks)}")
    dev = resolve_device(device)

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
    return {"masks": masks, "tasks": tasks, "dev": dev, "names": names, "mask_of": mask_of, "small_mask": small_mask,
            "in_dtype": in_dtype, "batches": batches, "declined": declined,
            "include_noise": bool(config.svd_include_noise)}


def _plan_tables(batch, setup, task_vectors, base_state_dict):
    """The device tables of one adopted plan for ``CompressPlan.project_tasks`` (and the extension entry points, which
    take the same ones): {"table", "base_table", "index_table", "rows_dev", "active", "keep"}.  ``active[i]``: entry i of
    the plan is projected; ``keep``: the owners of the raw addresses in the tables."""
    from . import mask_loader as ml
    from .pipeline import prepare_input
    tasks, dev, mask_of, in_dtype = setup["tasks"], setup["dev"], setup["mask_of"], setup["in_dtype"]
    include_noise = setup["include_noise"]
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
    keep.append(ms)
    return {"table": table, "base_table": base_table, "index_table": index_table, "rows_dev": rows_dev,
            "active": active, "keep": keep}


def _per_parameter_rest(rest, out, task_vectors, setup, bases, config, device, base_state_dict):
    """The per-parameter route (``compress_parameter``) for whatever did not go into a plan."""
    dev, masks = setup["dev"], setup["masks"]
    quantizer = RTVQQuantizer(num_bits=config.svd_low_bits, num_stages=config.svd_rtvq_stages)
    for name in rest:
        tv = task_vectors
        if base_state_dict is not None:
            b = base_state_dict[name]
            tv = {t: {name: (v[name].to(dev).float() - b.to(dev).float())} for t, v in task_vectors.items()
                  if name in v}
        comp = compress_parameter(name, tv, masks.get(name), bases[name], quantizer,
                                  include_noise=setup["include_noise"], min_mask_size=config.svd_min_mask_size,
                                  device=device)
        if comp is not None:
            out[name] = comp


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
    from .pipeline import task_artifact
    if not task_vectors:
        return {}
    setup = _projection_setup(task_vectors, masks, bases, config, device, base_state_dict, "project_all_parameters")
    tasks, dev = setup["tasks"], setup["dev"]

    out: Dict[str, Dict] = {}
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.device(dev):
            for batch in setup["batches"]:
                plan = batch.plan
                tb = _plan_tables(batch, setup, task_vectors, base_state_dict)
                active = tb["active"]
                sm = plan.project_tasks(tb["table"], base_table=tb["base_table"], index_table=tb["index_table"],
                                        rows_dev=tb["rows_dev"])
                del tb
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
        rest = [n for n in setup["names"] if n not in out]
        if rest:
            _per_parameter_rest(rest, out, task_vectors, setup, bases, config, device, base_state_dict)
    finally:
        if gc_was_on:
            gc.enable()
    return {n: out[n] for n in sorted(out)}


# ---- the stored bases grown by what the new tasks add outside their span (include/svdq.h, svdq_plan_residual_gram)
def _regions(basis):
    """The (region key, artifact key, region basis) triples of one parameter's stored basis."""
    return [(rk, ak, basis[rk]) for rk, ak in (("masked", "masked"), ("noise", "unmasked"))
            if isinstance(basis, dict) and isinstance(basis.get(rk), dict)]


def check_extension_room(bases: Dict[str, Dict], n_new: int, n_stored_tasks: Optional[int] = None) -> None:
    """The ``ValueError``s of ``extend_bases``, from shapes and scalars alone (no GPU): at most ``MAX_NEW_TASKS`` new
    tasks per call, and for every stored region k + n_new <= 32, r + n_new <= 32 and N + n_new <= 32 -- an extended
    store must be adoptable again (a plan has at most 32 slots and r <= N)."""
    if not 1 <= n_new <= nat.MAX_NEW_TASKS:
        raise ValueError(f"extend_bases takes 1 to {nat.MAX_NEW_TASKS} new tasks per call, got {n_new}")
    if n_stored_tasks is not None and n_stored_tasks + n_new > nat.MAX_TASKS:
        raise ValueError(f"{n_stored_tasks} stored + {n_new} new tasks: at most {nat.MAX_TASKS} tasks in total")
    for name in sorted(bases):
        for rk, _, b in _regions(bases[name]):
            k = int(b["k"])
            r = k + (int(b["U_low"].shape[1]) if b["U_low"].dim() == 2 else 0)
            if k + n_new > nat.MAX_TASKS:
                raise ValueError(f"parameter {name!r} [{rk}]: k + new tasks = {k} + {n_new} > {nat.MAX_TASKS}")
            if r + n_new > nat.MAX_TASKS:
                raise ValueError(f"parameter {name!r} [{rk}]: r + new tasks = {r} + {n_new} > {nat.MAX_TASKS}")
            n_old = b.get("N")
            if n_old is not None and int(n_old) + n_new > nat.MAX_TASKS:
                raise ValueError(f"parameter {name!r} [{rk}]: {int(n_old)} stored + {n_new} new tasks: at most "
                                 f"{nat.MAX_TASKS} tasks in total")


def extended_basis_entry(basis: Dict, u_high_ext: torch.Tensor, lam, n_added: int) -> Dict:
    """One region's basis dictionary after m = len(lam) new columns: U_high' = ``u_high_ext`` [D, k + m] (the stored
    columns first), k' = k + m, singular_values' = [sigma[:k], sqrt(lam), sigma[k:]] -- NOT globally descending any more;
    its first k' entries are still the high columns --, energy_retained by the reference's formula on that vector
    (compute_energy_spectrum, cum[k' - 1]; basis.py:116-156), N' = N + ``n_added``.  U_low and mean are the same
    objects.  A pure function of its arguments (no GPU)."""
    from .basis import compute_energy_spectrum
    k = int(basis["k"])
    lam_t = torch.as_tensor(lam, dtype=torch.float64).reshape(-1)
    m = int(lam_t.numel())
    if tuple(u_high_ext.shape) != (int(basis["U_high"].shape[0]), k + m):
        raise ValueError(f"U_high' has shape {tuple(u_high_ext.shape)}, expected "
                         f"{(int(basis['U_high'].shape[0]), k + m)}")
    sv = torch.as_tensor(basis["singular_values"]).detach().cpu().float().reshape(-1)
    sv2 = torch.cat([sv[:k], lam_t.clamp_min(0).sqrt().float(), sv[k:]])
    out = dict(basis)
    out["U_high"] = u_high_ext
    out["k"] = k + m
    out["singular_values"] = sv2
    out["energy_retained"] = float(compute_energy_spectrum(sv2)[k + m - 1]) if k + m > 0 else 0.0
    if "N" in basis:
        out["N"] = int(basis["N"]) + int(n_added)
    return out


def pad_c_high(artifact: Optional[Dict], m: int) -> Optional[Dict]:
    """An OLD task's region artifact against a basis that gained m high columns: c_high' = [c_high, 0 ... 0] (fp16 holds
    the zeros exactly), c_low_quant the same object."""
    if artifact is None or m <= 0:
        return artifact
    out = dict(artifact)
    c = artifact["c_high_fp16"]
    out["c_high_fp16"] = torch.cat([c.reshape(-1), torch.zeros(m, dtype=c.dtype, device=c.device)])
    return out


def extend_bases(task_vectors: Dict[str, Dict[str, torch.Tensor]], masks: Optional[Dict[str, torch.Tensor]],
                 bases: Dict[str, Dict], config, device: str = "cuda",
                 base_state_dict: Optional[Dict[str, torch.Tensor]] = None, min_residual: float = 2.0 ** -12) -> Dict:
    """``project_all_parameters`` plus the directions the new tasks add OUTSIDE the span of the stored columns: per plan
    project -> residual Gram + eigen stage -> read the m values -> write U_high' (include/svdq.h,
    svdq_plan_residual_gram).  No other task's checkpoint is read and no stored column is recomputed.

    Arguments as ``project_all_parameters``; 1 to 8 new tasks per call, and every stored region needs k + M <= 32,
    r + M <= 32 and N + M <= 32 (``ValueError`` before anything runs).  ``min_residual``: a residual direction is kept
    when its norm exceeds ``min_residual`` times the largest |xc_j| of the entry.  The default 2^-12 sits 16 x above the
    worst-case fp32 noise of the residual, (r + 2) 2^-24 sqrt(r) <= 1.2e-5 |xc| at r = 32, and far below what a 4-bit
    c_low resolves.

    Returns {"bases": the bases in the reference layout -- entries with new columns replaced by
    ``extended_basis_entry``'s dictionaries (CPU tensors), every other entry the object that came in --, "compressed":
    the new tasks' artifacts, c_high' = fp16([coef[:k], d_j]) on extended entries, otherwise exactly
    ``project_all_parameters``', "columns": {(param, region): m} for every entry that went through a plan,
    "captured_energy": {task: 1 - sum |e|^2 / sum |xc|^2 over those entries} -- the share of the task's energy the STORED
    columns capture, i.e. what the plain route keeps --, "skipped": the parameters that stayed on the per-parameter
    route (what ``adopt_bases`` declines, masks under ``svd_min_mask_size``): projected as today, not extended}."""
    import gc
    from .pipeline import task_artifact
    tasks = list(task_vectors.keys())
    check_extension_room(bases, len(tasks))
    setup = _projection_setup(task_vectors, masks, bases, config, device, base_state_dict, "extend_bases")
    dev, M = setup["dev"], len(tasks)
    out: Dict[str, Dict] = {}
    new_bases = dict(bases)
    columns: Dict = {}
    e_sum = {t: 0.0 for t in tasks}
    x_sum = {t: 0.0 for t in tasks}
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.device(dev):
            for batch in setup["batches"]:
                plan = batch.plan
                tb = _plan_tables(batch, setup, task_vectors, base_state_dict)
                active = tb["active"]
                args = dict(base_table=tb["base_table"], index_table=tb["index_table"], rows_dev=tb["rows_dev"])
                sm = plan.project_tasks(tb["table"], **args)
                ext = plan.residual_gram(tb["table"], M, min_residual=min_residual, **args)
                udt = torch.float16 if plan.fp16 else torch.float32
                outs = [None] * plan.P
                for i in range(plan.P):
                    m = int(ext.m[i])
                    if active[i] and m > 0:
                        outs[i] = torch.empty((int(sm.rows[i]), int(sm.k[i]) + m), dtype=udt, device=dev)
                if any(o is not None for o in outs):
                    plan.extend_basis(tb["table"], M, outs, **args)
                del tb
                for i, (name, region) in enumerate(batch.entries):
                    art_key = "masked" if region == "masked" else "unmasked"
                    per_task = out.setdefault(name, {})
                    m = int(ext.m[i]) if active[i] else 0
                    present = [t for t, task in enumerate(tasks) if name in task_vectors[task]]
                    if active[i]:
                        columns[(name, region)] = m
                    if m > 0:
                        nb = dict(new_bases[name])
                        nb[region] = extended_basis_entry(bases[name][region], outs[i].cpu(), ext.lam[i, :m], len(present))
                        new_bases[name] = nb
                    for t in present:
                        task = tasks[t]
                        art = per_task.setdefault(task, {"masked": None, "unmasked": None})
                        if not active[i]:
                            continue
                        a = task_artifact(plan, sm, i, t)
                        if m > 0:
                            a = dict(a)
                            d = torch.from_numpy(ext.d[i, t, :m].copy()).half()
                            a["c_high_fp16"] = torch.cat([a["c_high_fp16"].reshape(-1), d])
                        art[art_key] = a
                        e_sum[task] += float(ext.enorm[i, t])
                        x_sum[task] += float(ext.xnorm[i, t])
        rest = [n for n in setup["names"] if n not in out]
        if rest:
            _per_parameter_rest(rest, out, task_vectors, setup, bases, config, device, base_state_dict)
    finally:
        if gc_was_on:
            gc.enable()
    captured = {t: (1.0 - e_sum[t] / x_sum[t]) if x_sum[t] > 0.0 else 1.0 for t in tasks}
    return {"bases": new_bases, "compressed": {n: out[n] for n in sorted(out)}, "columns": columns,
            "captured_energy": captured, "skipped": sorted(rest)}


# ---- a store brought back to the form a fresh compress run would give it (include/svdq.h, svdq_plan_consolidate_eig)
def stored_task_names(compressed_all: Dict[str, Dict]) -> list:
    """The task names the coefficient dictionaries hold, sorted."""
    return sorted({t for per_task in compressed_all.values() if isinstance(per_task, dict) for t in per_task})


def consolidate_task_list(compressed_all: Dict[str, Dict], tasks=None) -> list:
    """The kept task list of ``consolidate_bases``: ``tasks`` (None = every stored task), SORTED BY NAME -- the order
    ``adopt_artifacts``, ``task_gram_from_artifacts`` and the merge's weight rows use for a store's tasks, not the order
    of ``diagnostics["task_weights"]``.  It is the destination's slot order and so the order of the sum behind bbar; the
    artifacts are keyed by name, so nothing a consumer reads depends on it.  ``ValueError`` on a task the store does not
    hold and on an empty list; a pure function of its arguments (no GPU)."""
    stored = stored_task_names(compressed_all)
    kept = stored if tasks is None else sorted(set(tasks))
    for t in kept:
        if t not in stored:
            raise ValueError(f"task {t!r} is not in the store, which holds {stored}")
    if not kept:
        raise ValueError("no task to keep: consolidating a store needs at least one of its tasks")
    if len(kept) > nat.MAX_TASKS:
        raise ValueError(f"{len(kept)} tasks: at most {nat.MAX_TASKS}")
    return kept


def check_consolidate_room(bases: Dict[str, Dict]) -> None:
    """``ValueError`` for a stored region whose r columns and mean exceed the 33 rows of the rebase table (r + 1 > 33);
    from shapes and scalars alone (no GPU)."""
    for name in sorted(bases):
        for rk, _, b in _regions(bases[name]):
            r = int(b["k"]) + (int(b["U_low"].shape[1]) if b["U_low"].dim() == 2 else 0)
            if r + 1 > nat.MAX_TASKS + 1:
                raise ValueError(f"parameter {name!r} [{rk}]: r + 1 = {r} + 1 > {nat.MAX_TASKS + 1}")


def keep_row(entry_tasks, kept) -> list:
    """One row of the keep table: for every kept task its slot in ``entry_tasks`` (a plan entry's task order), -1 where
    the entry does not hold the task."""
    pos = {t: j for j, t in enumerate(entry_tasks)}
    return [pos.get(t, -1) for t in kept]


def unquantizable_slots(scale, zero_point, slots) -> list:
    """The slots of ``slots`` whose c_low the quantizer could not represent: a stage's scale is not finite or is 0, or its
    zero point is not finite (``scale`` / ``zero_point``: [N][S] of one entry).  The reference's affine quantizer has
    scale = (2^b - 1) / (max - min) with no guard (rtvq.py:17-18): a stage whose input has no range -- a single element, or
    residuals of an earlier stage that came out equal, which two elements do more often than not -- gives 1 / 0, and what
    it dequantizes to is NaN.  A pure function (numpy)."""
    import numpy as np
    sc, zp = np.asarray(scale, dtype=np.float32), np.asarray(zero_point, dtype=np.float32)
    return [j for j in slots if not (np.isfinite(sc[j]).all() and (sc[j] != 0).all() and np.isfinite(zp[j]).all())]


def promoted_entry(basis: Dict, coef, slots) -> Tuple[Dict, Dict]:
    """One region whose c_low the quantizer cannot represent, stored on the high side instead: U_high' = [U_high | U_low],
    an empty U_low, k' = r', energy_retained = 1 (every kept direction is a high one), and per slot of ``slots`` the
    artifact {c_high_fp16 = fp16(coef[slot][:r']), c_low_quant = the quantizer's empty payload} -- fp16 holds what an
    affine code without a range cannot (``extend_bases`` puts its new columns on the high side for the same reason).
    ``coef``: the entry's fp32 coefficients [N][N].  Returns (basis', {slot: artifact}); the inputs are not touched."""
    import numpy as np
    k, n_low = int(basis["k"]), int(basis["U_low"].shape[1])
    r = k + n_low
    out = dict(basis)
    out["U_high"] = torch.cat([basis["U_high"], basis["U_low"]], dim=1).contiguous()
    out["U_low"] = basis["U_low"][:, :0].contiguous()
    out["k"] = r
    out["energy_retained"] = 1.0 if r > 0 else 0.0
    arts = {}
    for j in slots:
        c = torch.from_numpy(np.ascontiguousarray(np.asarray(coef, dtype=np.float32)[j, :r])).half()
        arts[j] = {"c_high_fp16": c, "c_low_quant": None}
    return out, arts


def consolidate_bases(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict], config, tasks=None,
                      min_sigma: float = 0.0, device: str = "cuda") -> Dict:
    """Re-derive bases, rank, mean and coefficients of a store from its artifacts alone -- after ``extend_bases`` grew it,
    to drop tasks, or to take it to another ``svd_energy_threshold`` / ``svd_max_rank`` / ``svd_low_bits`` /
    ``svd_rtvq_stages`` / ``svd_center`` -- without the fine-tuned checkpoints and without materialising a task model
    (include/svdq.h, svdq_plan_consolidate_eig: per plan the store Gram, the eigen stage and the streaming rebase).

    ``compressed_all`` / ``bases``: whatever ``adopt_artifacts`` accepts (the dictionaries ``load_all_artifacts``
    returns, or a fused run's).  ``config``: the settings of the consolidated store.  ``tasks``: the tasks to keep
    (None = all).  ``min_sigma``: directions below ``min_sigma * sigma_0`` are dropped besides those below the noise
    floor of the stored Gram.  ``ValueError`` before any GPU work: an unknown task, an empty kept list, a stored region
    with r + 1 > 33.

    Returns {"bases", "compressed"} in the reference's dictionary layouts (ready for ``save_all_artifacts``; ``N``,
    ``singular_values`` -- descending again --, ``k`` and ``energy_retained`` set; signal and noise regions are entries
    of their own), "columns": {(param, region): (r, r')}, "dropped_energy": {(param, region): sum of the dropped
    eigenvalues}, "noise_floor": {(param, region): eta, the bound on the error of the stored Gram's K; directions are
    kept above 4 eta}, "promoted": {(param, region): (k' of the rank rule, r')} for regions whose c_low the quantizer
    could not represent for some kept task (``unquantizable_slots``) and which are therefore stored with all r' columns
    on the high side (``promoted_entry``) -- no store with non-finite coefficients is handed out; a coefficient that is
    non-finite even so raises ``NonFiniteInput`` --, "skipped": the parameters ``adopt_artifacts`` declines -- they stay on the per-parameter route, their
    artifacts are handed back as they came."""
    from .driver import adopt_artifacts
    from .merge import _batched_entry
    import numpy as np
    from .pipeline import CompressPlan, NonFiniteInput, basis_dict, task_artifact
    kept = consolidate_task_list(compressed_all, tasks)
    check_consolidate_room(bases)
    dev = resolve_device(device)
    a_bases, a_comp = adopt_artifacts(bases, compressed_all, config, device=dev)
    names = sorted(compressed_all.keys())
    jobs, skipped = {}, []      # id(plan) -> (plan batch, {entry index: (name, region)})
    for name in names:
        got = _batched_entry(name, a_comp, a_bases)
        if got is None:
            skipped.append(name)
            continue
        batch, i, meta = got
        jobs.setdefault(id(batch.plan), (batch, {}))[1][i] = (name, "masked")
        if meta["noise"] is not None:
            nb, j = meta["noise"]
            jobs.setdefault(id(nb.plan), (nb, {}))[1][j] = (name, "noise")
    new_bases = {n: bases[n] for n in bases if n in skipped or n not in compressed_all}
    new_comp: Dict[str, Dict] = {n: compressed_all[n] for n in skipped}
    columns, dropped, floor, promoted = {}, {}, {}, {}
    by_param = getattr(config, "svd_low_bits_by_param", None)
    with torch.cuda.device(dev):
        for batch, entries in jobs.values():
            src = batch.plan
            keep = [keep_row(batch.task_names[i], kept) if i in entries else [-1] * len(kept) for i in range(src.P)]
            bits = [int(by_param(batch.entries[i][0])) if by_param is not None else int(config.svd_low_bits)
                    for i in range(src.P)]
            dst = CompressPlan(src.rows, len(kept), energy_threshold=config.svd_energy_threshold,
                               max_rank=config.svd_max_rank, center=config.svd_center, fp16=src.fp16, low_bits=bits,
                               rtvq_stages=config.svd_rtvq_stages, device=dev, workspace=False)
            try:
                sm, tab = src.consolidate(dst, keep, min_sigma=min_sigma)
            except NonFiniteInput as e:
                bad = [f"{batch.entries[i][0]} [{batch.entries[i][1]}]" for i in e.indices]
                raise NonFiniteInput(e.indices, "consolidate_bases: the stored artifacts of " + ", ".join(bad) +
                                     " contain non-finite values") from None
            for i, (name, region) in entries.items():
                art_key = "masked" if region == "masked" else "unmasked"
                columns[(name, region)] = (int(batch.small.r[i]), int(tab.r[i]))
                dropped[(name, region)] = float(tab.dropped[i])
                floor[(name, region)] = float(tab.eta[i])
                entry = basis_dict(dst, sm, i)
                entry["N"] = sum(1 for s in keep[i] if s >= 0)      # the kept tasks that hold the region
                slots = [j for j in range(len(kept)) if keep[i][j] >= 0]
                rn, kn = int(tab.r[i]), int(tab.k[i])
                arts = {j: task_artifact(dst, sm, i, j) for j in slots}
                if rn > kn and unquantizable_slots(sm.scale[i], sm.zero_point[i], slots):
                    entry, high = promoted_entry(entry, sm.coef[i], slots)
                    for j in slots:      # the quantizer's own payload of an empty c_low, with this entry's settings
                        q = dict(arts[j]["c_low_quant"])
                        q.update(payloads=[], original_shape=torch.Size([0]))
                        arts[j] = {"c_high_fp16": high[j]["c_high_fp16"], "c_low_quant": q}
                    promoted[(name, region)] = (kn, rn)
                if not np.isfinite(sm.coef[i][slots, :rn]).all():
                    raise NonFiniteInput([i], f"consolidate_bases: {name} [{region}]: non-finite coefficients")
                new_bases.setdefault(name, {"masked": None, "noise": None})[region] = entry
                per_task = new_comp.setdefault(name, {})
                for j in slots:
                    per_task.setdefault(kept[j], {"masked": None, "unmasked": None})[art_key] = arts[j]
    return {"bases": new_bases, "compressed": {n: new_comp[n] for n in sorted(new_comp)}, "columns": columns,
            "dropped_energy": dropped, "noise_floor": floor, "promoted": promoted, "skipped": sorted(skipped)}
