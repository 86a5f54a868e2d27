"""
Fused Step 4 + Step 5 driver (reference cli.py:311-361 and cli.py:436-442): every parameter of a
model, masked and noise regions included, goes through ONE plan -- six kernel launches and one
small D2H copy for the whole model -- and comes back as the reference's ``bases`` and
``compressed_all`` dictionaries.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import _native as nat
from .pipeline import (BatchResult, CompressPlan, NonFiniteInput, basis_dict, native_input_dtype, pack_small,
                       prepare_input, prepare_vector, resolve_device, small_views, task_artifact)
from . import mask_loader as ml



# the mask-walk mode (svdq_compress_masked) serves regions that hold at least this share of their tensors' elements --
# below it, skipping rows through index lists reads less than walking past them -- and the task counts whose default
# kernels walk at full speed (N <= 16; above, the walk exists but runs the one-wave pass 2, measured 20-24 % behind the
# index lists that feed the two-wave kernels)
WALK_MIN_DENSITY = 0.5
WALK_MAX_TASKS = 16


def _resident(tensors, dev) -> bool:
    """All tensors already satisfy the ABI's input contract except (possibly) for their shape: fp32, contiguous, on
    ``dev``, 16-byte aligned -- then the plan can take their addresses as they are (pointer_table re-checks)."""
    f32 = torch.float32
    for t in tensors:
        if t.dtype is not f32 or t.device != dev or not t.is_contiguous() or t.requires_grad or t.data_ptr() & 15:
            return False
    return True


def build_bases(task_vectors: Dict[str, Dict[str, torch.Tensor]], combined_masks: Optional[Dict[str, torch.Tensor]],
                config, device="cuda", base_state: Optional[Dict[str, torch.Tensor]] = None,
                task_gram: Optional[bool] = None) -> Dict[str, Dict]:
    """Step 4 for all parameters.  Returns ``bases`` (reference layout: {param: {"masked": basis|None,
    "noise": basis|None}}), already cast to fp16 when ``config.svd_fp16`` (cli.py:354-361), with the
    coefficients of Step 5 attached for ``compress_all_parameters``.

    ``task_gram`` (default: ``config.svd_weighting == "cluster"``): every plan of unmasked parameters also leaves the
    uncentred task Gram of its tensors (svdq_plan_task_gram, a by-product of pass 1; the artifacts are byte-identical
    either way), recorded on its BatchResult for ``clustering.task_gram(..., bases=bases)``.

    Raises ``NonFiniteInput`` (a RuntimeError) naming each ``'parameter' [region]`` of a plan whose task deltas hold NaN
    or Inf among the rows processed -- where the reference's torch.linalg.svd raises (include/svdq.h,
    svdq_eig_rank_select)."""
    if task_gram is None:
        task_gram = getattr(config, "svd_weighting", None) == "cluster"
    dev = resolve_device(device)
    combined_masks = combined_masks or {}
    names = sorted({n for tv in task_vectors.values() for n in tv.keys()})
    if base_state is not None:   # compute_task_vector's eligibility (task_vector_loader.py:126-139)
        names = [n for n in names if n in base_state and base_state[n].is_floating_point()]
    tasks = list(task_vectors.keys())
    include_noise = bool(config.svd_include_noise)
    min_size = int(config.svd_min_mask_size)
    # optional partition of the parameters by code width (BASELINE config #5, "mixed 8-bit / 2-bit"): a callable
    # name -> bits on the config; the reference itself has one width per run (compress.py:180-183)
    bits_by_param = getattr(config, "svd_low_bits_by_param", None)

    # group regions by the number of tasks that have the parameter, the way to the rows and the input dtype (one plan
    # each).  A parameter whose task tensors (and base tensor) all have one half dtype is read as it is (no fp32 copy;
    # byte-identical outputs); any mix of dtypes, and every "walk" region, gets fp32 copies (prepare_vector).
    groups: Dict[Tuple[int, str, torch.dtype], List[dict]] = {}   # (tasks present, "plain" | "gather" | "walk", dtype)
    keep = []
    with torch.cuda.device(dev):
        masked_by_n: Dict[int, List[tuple]] = {}
        for name in names:
            present = [t for t in tasks if name in task_vectors[t]
                       and (base_state is None or task_vectors[t][name].shape == base_state[name].shape)]
            if not present:
                continue
            deltas = [task_vectors[t][name] for t in present]
            mask = combined_masks.get(name)
            if mask is not None and mask.shape == deltas[0].shape and mask.numel() > 0:
                masked_by_n.setdefault(len(present), []).append((name, present, deltas, mask))
            else:
                idt = native_input_dtype(deltas + ([base_state[name]] if base_state is not None else []))
                if idt is not torch.float32:
                    vs = [prepare_input(d, dev, idt) for d in deltas]
                else:
                    vs = [d if d.dim() == 1 else prepare_vector(d, dev) for d in deltas] if _resident(deltas, dev) \
                        else [prepare_vector(d, dev) for d in deltas]
                if vs[0].numel() == 0:
                    continue
                # with the by-product a plan's Gram columns must mean the same tasks for all its parameters
                groups.setdefault((tuple(present) if task_gram else len(present), "plain", idt), []).append(
                    {"name": name, "region": "masked", "tasks": present, "vectors": vs, "count": None,
                     "upper": vs[0].numel(), "min": 0, "src": deltas,
                     "base": prepare_input(base_state[name], dev, idt) if base_state is not None else None})
        # Masked parameters never get compacted copies of their deltas.  One count + scan per group (mask.sum() stays
        # on the device and becomes rows_dev); then, per region, one of two ways to reach the selected rows:
        #   walk   (N <= 16 and the region holds at least half of the elements): both passes walk the source rows with
        #          the mask byte beside them and compact in LDS (svdq_compress_masked) -- nothing is built per row;
        #   gather (sparse regions, N > 16): int32 index lists, rows fetched through them (svdq_compress_gather).
        for n_present, items in masked_by_n.items():
            numels = [it[3].numel() for it in items]
            ms = ml.MaskSet(numels, dev)
            mask_list = [it[3] for it in items]
            ct, cf = ms.count_scan(mask_list)
            dens = float(ct.sum().item()) / float(max(sum(numels), 1))
            can_walk = n_present <= WALK_MAX_TASKS
            walk_sig = can_walk and dens >= WALK_MIN_DENSITY
            walk_noise = can_walk and include_noise and (1.0 - dens) >= WALK_MIN_DENSITY
            it_ = if_ = None
            if not walk_sig or (include_noise and not walk_noise):
                it_, if_, _, _ = ms.indices(mask_list, want_false=include_noise and not walk_noise)
            keep.append((ms, it_, if_))
            for q, (name, present, deltas, mask_q) in enumerate(items):
                ident = (mask_q.data_ptr(), mask_q.numel(), str(mask_q.device), mask_q.dtype)
                base_t = base_state[name] if base_state is not None else None
                native = native_input_dtype(deltas + ([base_t] if base_t is not None else []))
                prepared = {}

                def inputs(walk, deltas=deltas, base_t=base_t, native=native, prepared=prepared):
                    # the walk reads fp32 only; the index lists read fp16 / bf16 as they are
                    idt = torch.float32 if walk else native
                    if idt not in prepared:
                        prepared[idt] = ([prepare_input(d, dev, idt) for d in deltas],
                                         prepare_input(base_t, dev, idt) if base_t is not None else None)
                    return (idt,) + prepared[idt]

                idt, vs, bvec = inputs(walk_sig)
                e = {"name": name, "region": "masked", "tasks": present, "vectors": vs, "count": ct[q:q + 1],
                     "upper": vs[0].numel(), "min": min_size, "base": bvec, "src": deltas}
                e.update(ms=ms, q=q, inv=False, mask_ident=ident)
                if not walk_sig:
                    e["index"] = it_[q]
                groups.setdefault((n_present, "walk" if walk_sig else "gather", idt), []).append(e)
                if include_noise:
                    idt, vs, bvec = inputs(walk_noise)
                    e = {"name": name, "region": "noise", "tasks": present, "vectors": vs, "count": cf[q:q + 1],
                         "upper": vs[0].numel(), "min": 1, "gate": ct[q:q + 1], "base": bvec, "src": deltas}
                    e.update(ms=ms, q=q, inv=True, mask_ident=ident)
                    if not walk_noise:
                        e["index"] = if_[q]
                    groups.setdefault((n_present, "walk" if walk_noise else "gather", idt), []).append(e)
        order = {n: i for i, n in enumerate(names)}
        for lst in groups.values():
            lst.sort(key=lambda e: (order[e["name"]], e["region"] != "masked"))

        bases: Dict[str, Dict] = {}
        for (n_tasks, mode, idt), entries in groups.items():
            entries = [e for e in entries if e["upper"] > 0]
            if not entries:
                continue
            want_gram = bool(task_gram) and mode == "plain"
            if isinstance(n_tasks, tuple):
                n_tasks = len(n_tasks)
            plan = CompressPlan([e["upper"] for e in entries], n_tasks,
                                energy_threshold=config.svd_energy_threshold, max_rank=config.svd_max_rank,
                                center=config.svd_center, fp16=config.svd_fp16,
                                low_bits=([int(bits_by_param(e["name"])) for e in entries] if bits_by_param
                                          else config.svd_low_bits),
                                rtvq_stages=config.svd_rtvq_stages, device=dev, input_dtype=idt,
                                **({"task_gram": True} if want_gram else {}))
            rows_dev = None
            if any(e["count"] is not None for e in entries):
                # rows actually processed = mask.sum() (device), or 0 when below svd_min_mask_size
                parts = []
                for e in entries:
                    if e["count"] is None:
                        parts.append(torch.tensor([e["upper"]], dtype=torch.int64, device=dev))
                    else:
                        c = e["count"]
                        ok = c >= e["min"]
                        if "gate" in e:      # the noise region is only built when the signal region is (cli.py:332-338)
                            ok = ok & (e["gate"] >= min_size)
                        parts.append(torch.where(ok, c, torch.zeros_like(c)))
                rows_dev = torch.cat(parts)
            table = plan.pointer_table([e["vectors"] for e in entries])
            btab = None
            if base_state is not None:
                btab = torch.tensor([e["base"].data_ptr() for e in entries], dtype=torch.int64).to(dev)
                keep.append([e["base"] for e in entries])
            mtab = us = None
            if mode in ("walk", "gather"):
                # one source start per work unit: the walk mode's way to the rows, and what the batched consumers
                # (svdq_merge_masked / svdq_diagnostics_masked) put the merged rows back with, whichever mode compressed
                ms = entries[0]["ms"]
                mtab = torch.tensor([ms._s["mb"][e["q"]].data_ptr() for e in entries], dtype=torch.int64).to(dev)
                # the unit starts look a mask up by its index q in the mask set, the streaming kernels by plan entry:
                # two tables (they differ as soon as a plan holds both regions of a parameter)
                qtab = torch.tensor([b.data_ptr() for b in ms._s["mb"]], dtype=torch.int64).to(dev)
                us = ms.unit_starts(plan, rows_dev, entry_map=[(e["q"], e["inv"]) for e in entries], mask_table=qtab)
                keep.append((mtab, us))
            if mode == "walk":
                if btab is not None:
                    plan.run_masked_from_base(table, btab, mtab, us, rows_dev)
                else:
                    plan.run_masked(table, mtab, us, rows_dev)
            elif mode == "gather":
                itab = torch.tensor([e["index"].data_ptr() for e in entries], dtype=torch.int64).to(dev)
                if btab is not None:
                    plan.run_gather_from_base(table, btab, itab, rows_dev)
                else:
                    plan.run_gather(table, itab, rows_dev)
            elif btab is not None:
                plan.run_from_base(table, btab, rows_dev)
            else:
                plan.run(table, rows_dev)
            gram = plan.compress_task_gram() if want_gram else None
            try:
                small = plan.fetch_small()
            except NonFiniteInput as exc:
                # where the reference's torch.linalg.svd stops (basis.py:216-249, reached from cli.py Step 4); regions
                # the min-mask-size gate skips have rows_dev == 0, are never read and so never flagged
                where = ", ".join(f"{entries[i]['name']!r} [{entries[i]['region']}]" for i in exc.indices)
                raise NonFiniteInput(exc.indices, "input matrix contained non-finite values: the task deltas of "
                                     f"{where} hold NaN or Inf (parameter [region])") from exc
            batch = BatchResult(plan, small, [(e["name"], e["region"]) for e in entries],
                                [e["tasks"] for e in entries])
            batch.keep = keep
            # for the batched consumers (svdq_diagnostics reads the deltas again): what the run was launched with
            batch.mode, batch.table, batch.rows_dev = mode, table, rows_dev
            batch.mask_table, batch.unit_start = mtab, us
            batch.mask_ident = {e["name"]: e["mask_ident"] for e in entries if "mask_ident" in e}
            batch.from_base = base_state is not None
            # a from-base batch keeps its base table beside the fine-tuned one, and which of the caller's tensors each
            # device tensor was prepared from: the diagnostics from checkpoints (svdq_diagnostics_from_base) read them again
            batch.base_table = btab
            batch.sources = None
            if base_state is not None:
                batch.sources = {id(s): (s, v) for e in entries
                                 for s, v in zip(e["src"] + [base_state[e["name"]]], e["vectors"] + [e["base"]])}
            # the by-product: Gram of this plan's tensors, its task order, the parameters it covers
            batch.task_gram = ({"gram": gram, "tasks": list(entries[0]["tasks"]), "names": [e["name"] for e in entries]}
                               if want_gram else None)
            for i, e in enumerate(entries):
                slot = bases.setdefault(e["name"], {"masked": None, "noise": None})
                if int(small.rows[i]) <= 0:
                    continue
                # the views into the packed basis buffer are made when somebody looks at them
                slot[e["region"]] = LazyArtifacts((lambda pl=plan, sm=small, q=i: basis_dict(pl, sm, q)), (batch, i))
    # parameters whose masked region was skipped (mask.sum() < svd_min_mask_size) have no basis
    # entry at all in the reference (cli.py:343 guards the assignment)
    return {n: b for n, b in bases.items() if b["masked"] is not None}


class LazyArtifacts(dict):
    """A dictionary of one parameter -- {task: {"masked": art|None, "unmasked": art|None}} in ``compressed_all``, or a
    basis {U_high, U_low, singular_values, k, mean, energy_retained, D, N} in ``bases`` -- assembled from the packed
    buffers of the batched run on first access.  It IS a dict (isinstance, iteration, json, equality all behave); a caller that only
    passes the structure on (or inspects a few parameters) does not pay for assembling ~10^4 nested payload
    dictionaries per model.  storage.save_compressed_coefficients writes plain dicts (as the reference's writer
    does: it rebuilds the per-task level); pickled / torch.saved directly it comes back as a collections.OrderedDict,
    the one mapping type the weights-only unpickler admits besides dict itself."""
    __slots__ = ("_fill", "_batch", "_meta")

    def __init__(self, fill, batch=None, meta=None):
        super().__init__()
        self._fill = fill
        self._batch = batch      # (BatchResult, index): where this parameter's results live
        self._meta = meta        # compressed_all entries: which tasks / noise entry, for the batched consumers

    def _ensure(self):
        f = self._fill
        if f is not None:
            self._fill = None
            super().update(f())

    def __reduce__(self):
        from collections import OrderedDict
        self._ensure()
        return (OrderedDict, (), None, None, iter(dict.items(self)))

    def __repr__(self):
        self._ensure()
        return super().__repr__()


_MUTATORS = frozenset(("__setitem__", "__delitem__", "__ior__", "pop", "popitem", "setdefault", "update", "clear"))


def _lazy(name):
    def method(self, *a, **kw):
        self._ensure()
        for x in a:      # dict.__eq__ / __or__ / update read the OTHER operand through the C dict API, past its wrappers
            if isinstance(x, LazyArtifacts):
                x._ensure()
        if name in _MUTATORS:
            # an edited dictionary no longer describes the buffers of the fused run: the batched consumers (svdq_merge,
            # svdq_diagnostics) must not answer for it from there -- they fall back to the per-parameter route, which
            # reads the dictionary as the reference does
            self._batch = None
            self._meta = None
        return getattr(dict, name)(self, *a, **kw)
    method.__name__ = name
    return method


for _n in ("__getitem__", "__iter__", "__len__", "__contains__", "__eq__", "__ne__", "__setitem__", "__delitem__",
           "__or__", "__ror__", "__ior__", "__reversed__", "keys", "values", "items", "get", "pop", "popitem",
           "setdefault", "update", "copy", "clear", "__bool__" if hasattr(dict, "__bool__") else "__len__"):
    setattr(LazyArtifacts, _n, _lazy(_n))


def artifacts_from_batch(name: str, basis: Dict, task_vectors, config) -> Optional[Dict]:
    """{task: {"masked": art|None, "unmasked": art|None}} from the fused run, or None if this basis
    did not come from ``build_bases`` (then compress.py runs the per-task route)."""
    bm = basis.get("masked")
    if bm is None or getattr(bm, "_batch", None) is None:
        return None
    batch, i = bm._batch
    want_bits = getattr(config, "svd_low_bits_by_param", None)
    want_bits = int(want_bits(name)) if want_bits else config.svd_low_bits
    if (batch.plan.bits_of(i), batch.plan.S) != (want_bits, config.svd_rtvq_stages):
        return None
    tasks_i = batch.task_names[i]
    bn = basis.get("noise") if config.svd_include_noise else None
    have = [t for t in task_vectors.keys() if name in task_vectors[t]]

    def fill():
        out = {}
        pos = {t: j for j, t in enumerate(tasks_i)}
        npos = None
        if bn is not None and getattr(bn, "_batch", None) is not None:
            nb, j = bn._batch
            npos = {t: q for q, t in enumerate(nb.task_names[j])}
        for t in have:
            art = {"masked": None, "unmasked": None}
            if t in pos:
                art["masked"] = task_artifact(batch.plan, batch.small, i, pos[t])
            if npos is not None and t in npos:
                art["unmasked"] = task_artifact(nb.plan, nb.small, j, npos[t])
            out[t] = art
        return out

    return LazyArtifacts(fill, batch=bm._batch,
                         meta={"have": have, "tasks": tasks_i,
                               "noise": bn._batch if (bn is not None and getattr(bn, "_batch", None) is not None) else None})


def run_basis_and_compress(task_vectors, combined_masks, config, device="cuda", task_gram: Optional[bool] = None
                           ) -> Tuple[Dict, Dict]:
    """cli.py Step 4 + Step 5 in one call: (bases, compressed_all).  ``task_gram``: see ``build_bases``."""
    from .compress import compress_all_parameters
    bases = build_bases(task_vectors, combined_masks, config, device, task_gram=task_gram)
    return bases, compress_all_parameters(task_vectors, combined_masks or {}, bases, config, device)


def run_basis_and_compress_from_checkpoints(base_state: Dict[str, torch.Tensor],
                                            finetuned_states: Dict[str, Dict[str, torch.Tensor]], config,
                                            device="cuda", combined_masks: Optional[Dict[str, torch.Tensor]] = None,
                                            task_gram: Optional[bool] = None) -> Tuple[Dict, Dict]:
    """cli.py Step 1 + Step 4 + Step 5 without materialising the task vectors: ``finetuned - base`` is formed
    inside the two streaming passes (svdq_compress_from_base; with ``combined_masks`` the masked parameters go
    through svdq_compress_gather_from_base).  Same (bases, compressed_all) as load_task_vectors +
    run_basis_and_compress, bit for bit.  With ``task_gram`` (see ``build_bases``) the recorded Gram is that of the
    deltas formed in registers, so a cluster-weighted run needs no task vectors either."""
    from .compress import compress_all_parameters
    bases = build_bases(finetuned_states, combined_masks, config, device, base_state=base_state, task_gram=task_gram)
    return bases, compress_all_parameters(finetuned_states, combined_masks or {}, bases, config, device)


# ------------------------------------------------------------------------------------------------ stored artifacts
_REGIONS = (("masked", "masked"), ("noise", "unmasked"))      # (key in a basis file, key in a task's artifact)


def _basis_adoptable(basis, n: Optional[int] = None) -> Optional[str]:
    """Why the stored BASIS of one region cannot go into a plan, or None when it can -- the basis half of ``_adoptable``,
    and all of it for ``adopt_bases``.  ``n``: the tasks that hold the region (k + n_low may not exceed it), or None when
    the plan's task count is still free (then the library's limit bounds k + n_low).  Shapes, dtypes and scalars only."""
    if not isinstance(basis, dict):
        return "the basis is not a dictionary"
    uh, ul, k = basis.get("U_high"), basis.get("U_low"), basis.get("k")
    if not (isinstance(uh, torch.Tensor) and isinstance(ul, torch.Tensor) and uh.dim() == 2 and ul.dim() == 2):
        return "U_high / U_low are not matrices"
    if uh.dtype != ul.dtype:
        return "U_high and U_low have different dtypes"
    if uh.dtype not in (torch.float16, torch.float32):
        return f"basis dtype {uh.dtype} is neither fp16 nor fp32"
    D = int(uh.shape[0])
    if D < 1 or int(ul.shape[0]) != D or int(basis.get("D", D)) != D:
        return "U_high, U_low and D disagree on the row count"
    if isinstance(k, bool) or not isinstance(k, int) or int(uh.shape[1]) != k:
        return "U_high.shape[1] != k"
    n_low = int(ul.shape[1])
    r = k + n_low
    if n is None:
        if r > min(D, nat.MAX_TASKS):
            return f"k + n_low exceeds min(D, {nat.MAX_TASKS})"
    elif r > min(D, n):
        return "k + n_low exceeds min(D, tasks that hold the region)"
    mean, sv = basis.get("mean"), basis.get("singular_values")
    if mean is not None and not (isinstance(mean, torch.Tensor) and mean.dtype is torch.float32 and mean.numel() == D):
        return "mean is not an fp32 tensor of D elements"
    if not (isinstance(sv, torch.Tensor) and sv.dim() == 1 and sv.is_floating_point()):
        return "singular_values is not a vector"
    return None


def _adoptable(basis, artifacts) -> Optional[str]:
    """Why the stored artifacts of ONE region of one parameter cannot be adopted into a plan (``adopt_artifacts``), or
    None when they can.  ``basis``: the region's basis dictionary (U_high, U_low, k, mean, ...); ``artifacts``: the
    region's artifact {c_high_fp16, c_low_quant} of every task that holds it, in plan order.  Reads shapes, dtypes and
    scalars only -- no tensor data, no GPU."""
    n = len(artifacts)
    if n < 1:
        return "no task holds the region"
    if n > nat.MAX_TASKS:
        return f"more than {nat.MAX_TASKS} tasks"
    why = _basis_adoptable(basis, n)
    if why is not None:
        return why
    k, n_low = basis["k"], int(basis["U_low"].shape[1])
    r = k + n_low
    bits = stages = None
    for a in artifacts:
        if not isinstance(a, dict):
            return "a task's artifact is not a dictionary"
        ch, q = a.get("c_high_fp16"), a.get("c_low_quant")
        if not (isinstance(ch, torch.Tensor) and ch.dtype is torch.float16 and ch.dim() == 1 and ch.numel() == k):
            return "c_high_fp16 is not an fp16 row of k elements"
        if not isinstance(q, dict):
            return "c_low_quant is not a dictionary"
        b, s, shape, pays = q.get("num_bits"), q.get("num_stages"), q.get("original_shape"), q.get("payloads")
        if not isinstance(b, int) or not 1 <= b <= 8:
            return "num_bits outside 1..8"
        if not isinstance(s, int) or not 1 <= s <= nat.MAX_STAGES:
            return f"num_stages outside 1..{nat.MAX_STAGES}"
        if bits is None:
            bits, stages = b, s
        elif (b, s) != (bits, stages):
            return "the tasks disagree on num_bits / num_stages"
        if shape is None or len(shape) != 1 or k + int(shape[0]) != r:
            return "k + n_low != U_high.shape[1] + U_low.shape[1]"
        if not isinstance(pays, (list, tuple)) or len(pays) != (s if n_low > 0 or pays else 0):
            return "payload count != num_stages"
        for pl in pays:
            if not isinstance(pl, dict):
                return "a payload is not a dictionary"
            qz, sc, zp = pl.get("quantized"), pl.get("scale"), pl.get("zero_point")
            if not (isinstance(qz, torch.Tensor) and qz.dtype is torch.uint8 and qz.numel() == n_low):
                return "a quantized row is not uint8 of n_low elements"
            for x in (sc, zp):
                if not (isinstance(x, torch.Tensor) and x.dtype is torch.float32 and x.numel() == 1):
                    return "scale / zero_point is not one fp32 value"
    return None


def _adoption_groups(bases, compressed_all):
    """The GPU-free half of ``adopt_artifacts`` -- and, with ``compressed_all`` None, of ``adopt_bases``: the bases alone
    are grouped, by (basis dtype, mean is None), entries without tasks or artifacts and ``bits`` None --: which
    (parameter, region) pairs go into which plan.  Returns
    ``(groups, declined)``: groups = {(tasks present, num_stages, basis dtype, mean is None): [entry]} with entry =
    {name, region, art_key, basis, tasks, artifacts, bits}, in the dictionaries' order; declined = {name: reason}.  A
    parameter is adopted with ALL its regions or not at all (the batched consumers take both regions of a parameter
    from plans, or neither); a task that lacks a region is simply not among that entry's tasks, as in ``build_bases``."""
    groups: Dict[Tuple, List[dict]] = {}
    declined: Dict[str, str] = {}
    basis_only = compressed_all is None
    for name, b in bases.items():
        per_task = None if basis_only else compressed_all.get(name)
        if not isinstance(b, dict) or not (basis_only or isinstance(per_task, dict)):
            declined[name] = "no basis / coefficient dictionaries"
            continue
        if isinstance(per_task, LazyArtifacts) and per_task._batch is not None:
            declined[name] = "already backed by a plan"
            continue
        if b.get("masked") is None:
            declined[name] = "no masked basis"
            continue
        found, why = [], None
        for region, art_key in _REGIONS:
            rb = b.get(region)
            if rb is None:
                continue
            if basis_only:
                try:
                    why = _basis_adoptable(rb)
                except Exception as exc:
                    why = f"malformed ({type(exc).__name__})"
                if why is not None:
                    why = f"[{region}] {why}"
                    break
                found.append(((rb["U_high"].dtype, rb.get("mean") is None),
                              {"name": name, "region": region, "art_key": art_key, "basis": rb, "tasks": [],
                               "artifacts": [], "bits": None}))
                continue
            present = [(t, a[art_key]) for t, a in per_task.items() if isinstance(a, dict) and a.get(art_key) is not None]
            try:
                why = _adoptable(rb, [a for _, a in present])
            except Exception as exc:      # adoption never raises on data: whatever is malformed goes per parameter
                why = f"malformed ({type(exc).__name__})"
            if why is not None:
                why = f"[{region}] {why}"
                break
            q0 = present[0][1]["c_low_quant"]
            found.append(((len(present), int(q0["num_stages"]), rb["U_high"].dtype, rb.get("mean") is None),
                          {"name": name, "region": region, "art_key": art_key, "basis": rb,
                           "tasks": [t for t, _ in present], "artifacts": [a for _, a in present],
                           "bits": int(q0["num_bits"])}))
        if why is not None:
            declined[name] = why
            continue
        for key, e in found:
            groups.setdefault(key, []).append(e)
    return groups, declined


class _AdoptedViews:
    """What ``pipeline.task_artifact`` hands out for an adopted plan: the caller's own artifact dictionaries."""

    def __init__(self, artifacts):
        self.artifacts = artifacts


def _host_arrays(tensors):
    """numpy copies of many small tensors with one device-to-host copy per (device, dtype) instead of one per tensor
    (artifacts loaded with ``device="cuda"`` hold ~10^4 payload tensors per model)."""
    import numpy as np
    out = [None] * len(tensors)
    by_home: Dict[Tuple, List[int]] = {}
    for i, t in enumerate(tensors):
        if t.device.type == "cpu":
            out[i] = t.detach().reshape(-1).numpy()
        else:
            by_home.setdefault((t.device, t.dtype), []).append(i)
    for idx in by_home.values():
        flat = torch.cat([tensors[i].detach().reshape(-1) for i in idx]).cpu().numpy()
        pos = 0
        for i in idx:
            n = tensors[i].numel()
            out[i] = flat[pos:pos + n]
            pos += n
    return out


def _gather_each(entries, N: int, S: int) -> List[dict]:
    """The ``pack_small`` entries of one plan, tensor by tensor (any shapes and devices ``_adoptable`` lets through)."""
    import numpy as np
    flat, packed = [], []
    for e in entries:
        flat.append(e["basis"]["singular_values"])
        for a in e["artifacts"]:
            flat.append(a["c_high_fp16"])
            for pl in a["c_low_quant"]["payloads"]:
                flat += [pl["quantized"], pl["scale"], pl["zero_point"]]
    host = iter(_host_arrays(flat))
    for e in entries:
        b = e["basis"]
        k, n_low = int(b["k"]), int(b["U_low"].shape[1])
        sig = np.asarray(next(host), dtype=np.float32).reshape(-1)
        sigma = np.zeros(k + n_low, dtype=np.float32)
        sigma[:min(sig.size, k + n_low)] = sig[:k + n_low]
        ch = np.zeros((N, k), dtype=np.float16)
        codes = np.zeros((N, S, n_low), dtype=np.uint8)
        sc, zp, rn = (np.zeros((N, S), dtype=np.float32) for _ in range(3))
        for t, a in enumerate(e["artifacts"]):
            ch[t] = next(host)
            for s_, pl in enumerate(a["c_low_quant"]["payloads"]):
                codes[t, s_] = next(host)
                sc[t, s_] = next(host)[0]
                zp[t, s_] = next(host)[0]
                rn[t, s_] = np.float32(pl.get("residual_norm", 0.0))
        packed.append({"rows": int(b["U_high"].shape[0]), "k": k, "r": k + n_low,
                       "energy": b.get("energy_retained", 0.0), "sigma": sigma, "c_high": ch, "codes": codes,
                       "scale": sc, "zero_point": zp, "residual_norm": rn})
    return packed


def _gather_bulk(entries, N: int, S: int) -> List[dict]:
    """The same from ONE concatenation per field (and one device-to-host copy each when the artifacts were loaded onto
    the GPU): a model's ~17 000 payload tensors cost 9 us each when taken to numpy one by one, more than everything else
    in adoption together.  Needs what the writers produce -- 1-D rows, scales of one shape, every task of a parameter
    with all its stages or (no low columns) none; raises otherwise, and ``_gather_small`` goes tensor by tensor."""
    import numpy as np

    def host(ts, dtype, join=torch.cat):
        if not ts:
            return np.zeros(0, dtype=dtype)
        return join(ts).reshape(-1).cpu().numpy().astype(dtype, copy=False)

    arts = [a for e in entries for a in e["artifacts"]]
    pays = [pl for a in arts for pl in a["c_low_quant"]["payloads"]]
    sig = [e["basis"]["singular_values"] for e in entries]
    sigma = host(sig, np.float32)
    ch = host([a["c_high_fp16"] for a in arts], np.float16)
    qz = host([pl["quantized"] for pl in pays], np.uint8)
    sc = host([pl["scale"] for pl in pays], np.float32, torch.stack)
    zp = host([pl["zero_point"] for pl in pays], np.float32, torch.stack)
    rn = np.array([pl.get("residual_norm", 0.0) for pl in pays], dtype=np.float32)
    packed, i_sig, i_ch, i_qz, i_pl = [], 0, 0, 0, 0
    for e, sv in zip(entries, sig):
        b = e["basis"]
        k, n_low = int(b["k"]), int(b["U_low"].shape[1])
        r = k + n_low
        counts = {len(a["c_low_quant"]["payloads"]) for a in e["artifacts"]}
        if len(counts) != 1:
            raise ValueError("the tasks of a parameter differ in their number of payloads")
        stages = counts.pop()
        n_sv = int(sv.numel())
        sg = np.zeros(r, dtype=np.float32)
        sg[:min(n_sv, r)] = sigma[i_sig:i_sig + min(n_sv, r)]
        i_sig += n_sv
        codes = np.zeros((N, S, n_low), dtype=np.uint8)
        s_, z_, n_ = (np.zeros((N, S), dtype=np.float32) for _ in range(3))
        if stages:
            codes[:, :stages] = qz[i_qz:i_qz + N * stages * n_low].reshape(N, stages, n_low)
            s_[:, :stages] = sc[i_pl:i_pl + N * stages].reshape(N, stages)
            z_[:, :stages] = zp[i_pl:i_pl + N * stages].reshape(N, stages)
            n_[:, :stages] = rn[i_pl:i_pl + N * stages].reshape(N, stages)
        packed.append({"rows": int(b["U_high"].shape[0]), "k": k, "r": r, "energy": b.get("energy_retained", 0.0),
                       "sigma": sg, "c_high": ch[i_ch:i_ch + N * k].reshape(N, k), "codes": codes, "scale": s_,
                       "zero_point": z_, "residual_norm": n_})
        i_ch, i_qz, i_pl = i_ch + N * k, i_qz + N * stages * n_low, i_pl + N * stages
    if (i_sig, i_ch, i_qz, i_pl) != (sigma.size, ch.size, qz.size, sc.size) or sc.size != zp.size:
        raise ValueError("the concatenated fields do not have the sizes the shapes promise")
    return packed


def _gather_small(entries, N: int, S: int) -> List[dict]:
    try:
        return _gather_bulk(entries, N, S)
    except Exception:      # unusual shapes, tensors spread over devices: nothing is lost but time
        return _gather_each(entries, N, S)


def _device_source(t: Optional[torch.Tensor], dev, dtype) -> Optional[torch.Tensor]:
    """A source tensor of svdq_plan_import: on ``dev``, contiguous, 16-byte aligned; the tensor itself when it is."""
    if t is None or t.numel() == 0:
        return None
    v = t.detach()
    if v.device != dev or v.dtype is not dtype:
        v = v.to(device=dev, dtype=dtype)
    v = v.contiguous()
    return v.clone() if v.data_ptr() & 15 else v


def _planned_rows(entry, masks) -> int:
    """Rows an adopted entry is planned with: the stored D, or the element count of the caller's mask for it."""
    D = int(entry["basis"]["U_high"].shape[0])
    m = masks.get(entry["name"]) if masks else None
    return int(m.numel()) if isinstance(m, torch.Tensor) and m.numel() >= D else D


def _walk_usable(entries, q_of, plan_rows, stored_rows, numels, count_true, count_false) -> List[int]:
    """The mask-count check of ``adopted_mask_walk``, on host numbers: entry i = (name, region) can be walked with mask
    q_of[name] when the plan holds that mask's element count as its source rows and the mask selects -- set elements
    for "masked", cleared ones for "noise" -- exactly the stored rows."""
    ok = []
    for i, (name, region) in enumerate(entries):
        q = q_of.get(name)
        if q is None or int(stored_rows[i]) <= 0 or int(plan_rows[i]) != int(numels[q]):
            continue
        if int(count_false[q] if region == "noise" else count_true[q]) == int(stored_rows[i]):
            ok.append(i)
    return ok


def adopted_mask_walk(batch, masks):
    """For an ADOPTED batch and the caller's ``masks``: what the source-walk consumer (svdq_task_reconstruct_masked)
    puts compacted rows back with.  Masks are not stored (reference reload.py:204-205), so the tables a fused run
    keeps are built here: one MaskSet over the batch's masked parameters, one count + scan, ONE small device-to-host
    copy of the counts.  An entry is usable only if its counts equal the stored ``rows`` (``_walk_usable``); one whose
    mask does not fit keeps the compacted route, and so raises what it raises today.  Returns ``(mask_table [P],
    unit_start [plan units], usable entry indices)`` or None when nothing fits; cached on the batch by mask identity."""
    import numpy as np
    from . import mask_loader as ml
    plan, small = batch.plan, batch.small
    names = []
    for name, _ in batch.entries:
        m = masks.get(name) if masks else None
        if isinstance(m, torch.Tensor) and m.numel() > 0 and name not in names:
            names.append(name)
    if not names:
        return None
    ident = tuple((n, masks[n].data_ptr(), masks[n].numel(), str(masks[n].device), masks[n].dtype) for n in names)
    cached = getattr(batch, "_mask_walk", None)
    if cached is not None and cached[0] == ident:
        return cached[1]
    dev = plan.device
    result = None
    with torch.cuda.device(dev):
        numels = [int(masks[n].numel()) for n in names]
        ms = ml.MaskSet(numels, dev)
        ct, cf = ms.count_scan([masks[n] for n in names])
        counts = torch.stack([ct, cf]).cpu()
        q_of = {n: q for q, n in enumerate(names)}
        usable = _walk_usable(batch.entries, q_of, plan.rows, small.rows, numels, counts[0].tolist(), counts[1].tolist())
        if usable:
            rows = np.zeros(plan.P, dtype=np.int64)      # entries that do not fit: no unit of theirs is walked
            mtab = np.zeros(plan.P, dtype=np.int64)
            emap = [(0, False)] * plan.P
            for i in usable:
                name, region = batch.entries[i]
                rows[i] = int(small.rows[i])
                mtab[i] = ms._s["mb"][q_of[name]].data_ptr()
                emap[i] = (q_of[name], region == "noise")
            us = ms.unit_starts(plan, torch.from_numpy(rows).to(dev), entry_map=emap)
            result = (torch.from_numpy(mtab).to(dev), us, frozenset(usable))
    # the mask set owns the mask bytes the table points at; the caller's tensors are held so that their identity stays theirs
    batch._mask_walk = (ident, result, ms, [masks[n] for n in names])
    return result


def _adopt_plan(entries, N: int, S: int, udt, no_mean: bool, config, dev, masks, packed, bits, views=None,
                input_dtype=torch.float32):
    """One adopted plan -- shared by ``adopt_artifacts`` and ``adopt_bases``: a workspace-less ``CompressPlan`` over the
    entries' rows, its small buffer packed from ``packed`` (``pack_small`` entries) and the entries' U_high / U_low /
    mean copied into its packed buffers by ONE launch (svdq_plan_import).  Returns the ``BatchResult`` (mode "plain", no
    table, nothing kept), or None when the library has no plan for the set (SVDQ_EINVAL): those parameters stay as they
    came."""
    P = len(entries)
    try:
        plan = CompressPlan([_planned_rows(e, masks) for e in entries], N,
                            energy_threshold=config.svd_energy_threshold, max_rank=config.svd_max_rank,
                            center=not no_mean, fp16=udt is torch.float16, low_bits=list(bits),
                            rtvq_stages=S, device=dev, workspace=False, input_dtype=input_dtype)
    except ValueError:
        return None
    small_host = pack_small(plan.layout, P, N, S, packed)
    # the sources of the one copy launch; device copies of CPU tensors live until the end of this call only
    uh = [_device_source(e["basis"]["U_high"], dev, udt) for e in entries]
    ul = [_device_source(e["basis"]["U_low"], dev, udt) for e in entries]
    mn = None if no_mean else [_device_source(e["basis"]["mean"].reshape(-1), dev, torch.float32) for e in entries]
    plan.import_artifacts(uh, ul, mn, small_host)
    del uh, ul, mn
    small = small_views(small_host, plan.layout, P, N, S)
    if views is not None:
        small._host_views = views
    batch = BatchResult(plan, small, [(e["name"], e["region"]) for e in entries], [e["tasks"] for e in entries])
    batch.keep = None
    batch.mode, batch.table, batch.rows_dev = "plain", None, None
    batch.mask_table, batch.unit_start, batch.mask_ident = None, None, {}
    batch.from_base, batch.task_gram, batch.adopted = False, None, True
    batch.base_table, batch.sources = None, None
    plan._keep = None
    return batch


def _bases_plan_specs(bases, n_slots: int):
    """The GPU-free half of ``adopt_bases``: ``(specs, declined)`` with one spec per plan, {udt, no_mean, N, entries} --
    the groups of ``_adoption_groups`` over the bases alone, each with N = max(n_slots, the largest stored r of the
    group), so that r <= N holds for every entry and every plan has room for ``n_slots`` task slots."""
    n_slots = int(n_slots)
    if not 1 <= n_slots <= nat.MAX_TASKS:
        raise ValueError(f"n_slots must be in [1, {nat.MAX_TASKS}], got {n_slots}")
    groups, declined = _adoption_groups(bases, None)
    specs = []
    for (udt, no_mean), entries in groups.items():
        r_max = max(int(e["basis"]["k"]) + int(e["basis"]["U_low"].shape[1]) for e in entries)
        specs.append({"udt": udt, "no_mean": no_mean, "N": max(n_slots, r_max), "entries": entries})
    return specs, declined


def adopt_bases(bases: Dict[str, Dict], config, n_slots: int, device="cuda",
                masks: Optional[Dict[str, torch.Tensor]] = None, input_dtype=torch.float32):
    """Adoption of BASES only: stored bases -- loaded from disk, a caller's own U -- go into plans that have room for
    ``n_slots`` new tasks, ready for ``CompressPlan.project_tasks`` (svdq_plan_project).  The groups and plans are
    ``adopt_artifacts``' (same code), without the task count in the key: one plan per (basis dtype, mean is None) with
    N = max(n_slots, the largest stored r in the group) task slots, num_stages and the code widths from ``config``
    (``svd_low_bits_by_param`` respected).  U_high / U_low / mean / sigma / k / r / energy are imported, the coefficient
    fields are zero.  ``masks``: as for ``adopt_artifacts``; ``input_dtype``: the dtype the plans read task tensors in.
    Returns ``(batches, declined)``: the ``BatchResult`` of every plan (``entries`` = [(name, region)], in the
    dictionaries' order) and {name: reason} for what a plan cannot express -- those parameters stay with the
    per-parameter route.  Adoption never raises on data."""
    import numpy as np
    dev = resolve_device(device)
    specs, declined = _bases_plan_specs(bases, n_slots)
    S = int(config.svd_rtvq_stages)
    by_param = getattr(config, "svd_low_bits_by_param", None)
    batches = []
    for spec in specs:
        entries, N = spec["entries"], spec["N"]
        sig = _host_arrays([e["basis"]["singular_values"] for e in entries])
        packed, bits = [], []
        for e, sv in zip(entries, sig):
            b = e["basis"]
            k, n_low = int(b["k"]), int(b["U_low"].shape[1])
            r = k + n_low
            sigma = np.zeros(r, dtype=np.float32)
            sv = np.asarray(sv, dtype=np.float32).reshape(-1)
            sigma[:min(sv.size, r)] = sv[:r]
            packed.append({"rows": int(b["U_high"].shape[0]), "k": k, "r": r, "energy": b.get("energy_retained", 0.0),
                           "sigma": sigma, "c_high": np.zeros((N, k), dtype=np.float16),
                           "codes": np.zeros((N, S, n_low), dtype=np.uint8),
                           "scale": np.zeros((N, S), dtype=np.float32), "zero_point": np.zeros((N, S), dtype=np.float32),
                           "residual_norm": np.zeros((N, S), dtype=np.float32)})
            bits.append(int(by_param(e["name"])) if by_param is not None else int(config.svd_low_bits))
        batch = _adopt_plan(entries, N, S, spec["udt"], spec["no_mean"], config, dev, masks, packed, bits,
                            input_dtype=input_dtype)
        if batch is None:
            for e in entries:
                declined.setdefault(e["name"], "the library has no plan for this set")
            continue
        batches.append(batch)
    return batches, declined


def adopt_artifacts(bases: Dict[str, Dict], compressed_all: Dict[str, Dict], config, device="cuda",
                    masks: Optional[Dict[str, torch.Tensor]] = None) -> Tuple[Dict[str, Dict], Dict[str, Dict]]:
    """Put artifacts that did NOT come out of a fused run in this process -- the reference-layout dictionaries
    ``load_all_artifacts`` returns, tensors on the CPU or the GPU -- into plans, so that ``merge_all_parameters``,
    ``merge_with_clustering`` and ``reconstruct_from_artifacts`` serve them in two launches per plan (svdq_merge)
    instead of a payload upload, a dequantize launch and a reconstruct launch per (parameter, task).

    Returns ``(bases, compressed_all)``: new dictionaries with the same keys and the same values, field by field and
    dtype by dtype (the basis tensors now views of a plan's packed buffers on ``device``; the per-task artifact
    dictionaries the caller's own objects), whose entries are ``LazyArtifacts`` backed by adopted plans -- built as
    ``build_bases`` / ``artifacts_from_batch`` build theirs, with ``BatchResult.mode = "plain"`` and no table, unit
    starts or kept inputs: ``merge._batched_entry`` accepts them, masked parameters take the compacted-rows route with
    the CALLER's mask (masks are not stored: reference reload.py:204-205), the batched diagnostics skip them (there are
    no task vectors to measure against).  Assigning into an adopted entry sends that parameter back to the
    per-parameter route, as for a fused run's.

    One plan per (tasks that hold the region, num_stages, basis dtype, mean is None); "masked" and "noise" regions are
    entries of their own; ``num_bits`` is per parameter (svdq_plan_set_low_bits).  What a plan cannot express is
    declined silently, parameter by parameter, and handed back exactly as it came (``_adoptable`` lists the reasons:
    more than 32 tasks, shapes that disagree with k / n_low, other dtypes, ...), so the per-parameter route serves it
    as before.  Adoption never raises on data.

    ``masks``: the masks the caller will reconstruct with.  A masked parameter's entries are then planned with as many
    rows as its mask has elements (the stored D rows are what is filled and read), which is what the source walk of
    ``reconstruct_task_vectors_masked`` needs to put the rows back inside the launch
    (``adopted_mask_walk``); every other consumer reads the stored row counts and works as before.

    Memory: while a plan is being filled its sources and its packed copy coexist (4.9 GB twice at ViT-L-14 x 8).
    Plans are filled one after the other, and the device copies made of CPU tensors are dropped before the next plan;
    sources that already live on the device are read where they are and stay the caller's to release (drop the
    dictionaries that were passed in)."""
    dev = resolve_device(device)
    groups, _ = _adoption_groups(bases, compressed_all)
    new_bases = dict(bases)
    new_comp = dict(compressed_all)
    where: Dict[Tuple[str, str], Tuple[BatchResult, int]] = {}
    for (n_tasks, stages, udt, no_mean), entries in groups.items():
        batch = _adopt_plan(entries, n_tasks, stages, udt, no_mean, config, dev, masks,
                            _gather_small(entries, n_tasks, stages), [e["bits"] for e in entries],
                            views=_AdoptedViews([e["artifacts"] for e in entries]))
        if batch is None:
            continue
        for i, e in enumerate(entries):
            where[(e["name"], e["region"])] = (batch, i)
    for (name, region), (batch, i) in where.items():
        if new_bases[name] is bases[name]:
            new_bases[name] = dict(bases[name])
        orig = bases[name][region]

        def fill_basis(pl=batch.plan, sm=batch.small, q=i, orig=orig):
            d = basis_dict(pl, sm, q)
            out = dict(orig.items())      # the caller's keys, order and scalars; the tensors that now live in the plan
            out.update(U_high=d["U_high"], U_low=d["U_low"],
                       mean=d["mean"].view(orig["mean"].shape) if d["mean"] is not None else None)
            sv = orig["singular_values"]
            if sv.dtype is torch.float32 and sv.numel() == d["singular_values"].numel():
                out["singular_values"] = d["singular_values"]
            return out
        new_bases[name][region] = LazyArtifacts(fill_basis, (batch, i))
    for name in {n for n, _ in where}:
        per_task = compressed_all[name]
        mb, mi = where[(name, "masked")]
        new_comp[name] = LazyArtifacts((lambda d=per_task: dict(d.items())), batch=(mb, mi),
                                       meta={"have": list(per_task.keys()), "tasks": mb.task_names[mi],
                                             "noise": where.get((name, "noise"))})
    return new_bases, new_comp
