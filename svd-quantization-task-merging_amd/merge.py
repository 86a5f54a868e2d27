"""
Coefficient-space merge on the GPU with the reference's callables (SURVEY.md section 8 f1;
reference src/svd_hybrid/merge.py:61-552).  The heavy step -- U c + mean over every row of a
parameter -- is `svdq_reconstruct` (HBM-bound: reads the fp16 basis once, writes fp32); the masked
scatter is `svdq_mask_expand`.  Averaging N x N scalars per parameter is host-sized work on small
device tensors.  Weights come from weighting.py, cluster labels from clustering.py (Gram-based).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _native as nat
from .pipeline import prepare_vector, resolve_device, wants_cpu, _ptr, _stream_ptr
from .rtvq import RTVQQuantizer


def dequantize_and_average(compressed_coeffs: Dict[str, Dict], weights: Dict[str, float], quantizer: RTVQQuantizer,
                           region: str = "masked", device: str = "cpu"
                           ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Reference merge.py:61-141: tasks sorted by name, weights renormalised over present tasks."""
    names = sorted(compressed_coeffs.keys())
    highs, lows, ws = [], [], []
    for name in names:
        art = compressed_coeffs[name]
        if art is None or art.get(region) is None:
            continue
        ra = art[region]
        highs.append(ra["c_high_fp16"].to(device).float())
        lows.append(quantizer.dequantize(ra["c_low_quant"], device=device).float())
        ws.append(weights.get(name, 1.0 / len(names)))
    if not highs:
        return None, None
    tot = sum(ws)
    w = torch.tensor([x / tot for x in ws], device=device, dtype=torch.float32)
    # (stack * w).sum(0) task by task: rounded products added in task order -- the association the batched kernel
    # (k_merge_coeff) uses, so both routes give the same bits (torch's own reduction order depends on its launch shape)
    hi, lo = highs[0] * w[0], lows[0] * w[0]
    for j in range(1, len(highs)):
        hi = hi + highs[j] * w[j]
        lo = lo + lows[j] * w[j]
    return hi, lo


def reconstruct_from_coefficients(avg_c_high: torch.Tensor, avg_c_low: torch.Tensor, U_high: torch.Tensor,
                                  U_low: torch.Tensor, device: str = "cpu", mean: Optional[torch.Tensor] = None
                                  ) -> torch.Tensor:
    """Reference merge.py:144-194: U_high c_high + U_low c_low (+ mean); result on ``device`` (computed on the GPU)."""
    out = _reconstruct(avg_c_high, avg_c_low, U_high, U_low, mean, 1.0)
    return out.cpu() if wants_cpu(device) else out


def _reconstruct(avg_c_high, avg_c_low, U_high, U_low, mean, scale: float) -> torch.Tensor:
    """``scale`` folds the ``* noise_shrink`` of merge.py:284 into the same streaming pass."""
    lib = nat.lib()
    dev = resolve_device(U_high.device if U_high.is_cuda else "cuda")
    D = U_high.shape[0] if U_high.dim() == 2 else U_low.shape[0]
    k = U_high.shape[1] if U_high.dim() == 2 else 0
    nl = U_low.shape[1] if U_low.dim() == 2 else 0
    # fp16 kernels only when every array that has columns is fp16; a mix is lifted to fp32, never rounded down
    fp16 = k + nl > 0 and all(u.dtype == torch.float16 for u, n in ((U_high, k), (U_low, nl)) if n)
    dt = torch.float16 if fp16 else torch.float32
    uh = U_high.to(device=dev, dtype=dt).contiguous() if k else None
    ul = U_low.to(device=dev, dtype=dt).contiguous() if nl else None
    coef = torch.cat([avg_c_high.to(dev).float().reshape(-1), avg_c_low.to(dev).float().reshape(-1)]).contiguous()
    if coef.numel() != k + nl:
        raise ValueError(f"Shape mismatch: {coef.numel()} coefficients for {k + nl} basis columns")
    m = prepare_vector(mean.squeeze() if mean.dim() > 1 else mean, dev) if mean is not None else None
    out = torch.empty(D, dtype=torch.float32, device=dev)
    if D == 0:
        return out
    with torch.cuda.device(dev):
        if k + nl <= 32:
            nat.check(lib.svdq_reconstruct(_ptr(uh), _ptr(ul), int(fp16), D, k, nl, _ptr(coef), _ptr(m), float(scale),
                                           _ptr(out), _stream_ptr()), "svdq_reconstruct")
        else:
            # wider than the path ever is (N <= 32): column groups, each adding onto the running sum through the
            # kernel's `mean` input; the scale goes on last
            groups = [(u[:, c0:c0 + 32].contiguous(), off + c0, min(32, n - c0))
                      for u, n, off in ((uh, k, 0), (ul, nl, k)) if n for c0 in range(0, n, 32)]
            acc, dst = m, (out, torch.empty_like(out))     # input and output of a launch never alias
            for i, (u, c0, cn) in enumerate(groups):
                last = i == len(groups) - 1
                nat.check(lib.svdq_reconstruct(_ptr(u), _ptr(None), int(fp16), D, cn, 0, _ptr(coef[c0:c0 + cn]),
                                               _ptr(acc), float(scale) if last else 1.0, _ptr(dst[i % 2]),
                                               _stream_ptr()), "svdq_reconstruct")
                acc = dst[i % 2]
            out = acc
    return out


def merge_parameter(param_name: str, compressed_params: Dict[str, Dict], basis: Dict, weights: Dict[str, float],
                    quantizer: RTVQQuantizer, original_shape: torch.Size, mask: Optional[torch.Tensor] = None,
                    include_noise: bool = False, noise_shrink: float = 1.0, device: str = "cpu") -> torch.Tensor:
    """Reference merge.py:197-301."""
    from .mask_loader import reconstruct_from_masked
    dev = resolve_device(device)
    merged_masked = merged_unmasked = None
    bm = basis.get("masked")
    if bm is not None:
        ch, cl = dequantize_and_average(compressed_params, weights, quantizer, region="masked", device=dev)
        if ch is not None:
            merged_masked = reconstruct_from_coefficients(ch, cl, bm["U_high"], bm["U_low"], device=dev,
                                                          mean=bm.get("mean"))
    if include_noise:
        bu = basis.get("noise")
        if bu is not None:
            ch, cl = dequantize_and_average(compressed_params, weights, quantizer, region="unmasked", device=dev)
            if ch is not None:
                merged_unmasked = _reconstruct(ch, cl, bu["U_high"], bu["U_low"], bu.get("mean"), noise_shrink)
    if mask is not None and merged_masked is not None:
        res = reconstruct_from_masked(merged_masked, merged_unmasked, mask, original_shape)
    elif merged_masked is not None:
        res = merged_masked.view(original_shape)
    else:
        res = torch.zeros(original_shape, device=dev)
    return res.cpu() if wants_cpu(device) else res      # the reference returns on `device` (default "cpu")


def _batched_entry(name, compressed_all, bases):
    """(plan batch, index, meta) when both dictionaries of ``name`` still are what the fused run handed out: the
    LazyArtifacts themselves drop their handle on any edit through them; what an edit can reach WITHOUT going through
    them is checked here -- the noise entry of the (plain) per-parameter basis dictionary, and, once a compressed entry
    has been materialised, the per-task dictionaries it handed out (a deleted task, an artifact replaced or set to
    None).  In-place edits of payload tensors are not detectable; the reference has no such use."""
    from .driver import LazyArtifacts
    from .pipeline import task_artifact
    b, ca = bases.get(name), compressed_all.get(name)
    bm = b.get("masked") if isinstance(b, dict) else None
    if not (isinstance(bm, LazyArtifacts) and bm._batch is not None and isinstance(ca, LazyArtifacts)
            and ca._meta is not None and ca._batch is not None and ca._batch[0] is bm._batch[0]
            and ca._batch[1] == bm._batch[1]):
        return None
    meta = ca._meta
    bn = b.get("noise")
    if meta["noise"] is not None:
        if not (isinstance(bn, LazyArtifacts) and bn._batch is not None and bn._batch[0] is meta["noise"][0]
                and bn._batch[1] == meta["noise"][1]):
            return None
    elif bn is not None:
        return None
    if ca._fill is None:      # materialised: somebody may hold (and have edited) the per-task dictionaries
        batch, i = bm._batch
        if list(dict.keys(ca)) != list(meta["have"]):
            return None
        pos = {t: j for j, t in enumerate(batch.task_names[i])}
        npos = None
        if meta["noise"] is not None:
            nb, j = meta["noise"]
            npos = {t: q for q, t in enumerate(nb.task_names[j])}
        for t in meta["have"]:
            art = dict.__getitem__(ca, t)
            if not isinstance(art, dict):
                return None
            # a fused run hands out both keys; stored files hold only the regions a task has (storage.py:137-174), and
            # an adopted plan (driver.adopt_artifacts) answers with the caller's own artifact dictionaries
            if not (set(art.keys()) <= {"masked", "unmasked"} if getattr(batch, "adopted", False)
                    else set(art.keys()) == {"masked", "unmasked"}):
                return None
            want_m = task_artifact(batch.plan, batch.small, i, pos[t]) if t in pos else None
            want_u = task_artifact(nb.plan, nb.small, j, npos[t]) if (npos is not None and t in npos) else None
            if art.get("masked") is not want_m or art.get("unmasked") is not want_u:
                return None
    return bm._batch[0], bm._batch[1], meta


def _task_weights(have, tasks_i, members, weights):
    """One row of the weight table of k_merge_coeff: the reference's renormalised weights (merge.py:89-124) of the
    tasks of ``members`` (None = all) that have the parameter, in the plan's task order; -1 = not in the set."""
    import numpy as np
    names = sorted(t for t in have if members is None or t in members)
    present = [t for t in names if t in tasks_i]
    row = np.full(len(tasks_i), -1.0, dtype=np.float32)
    if not present:
        return row, False
    ws = [weights.get(t, 1.0 / len(names)) for t in present]
    tot = sum(ws)
    pos = {t: j for j, t in enumerate(tasks_i)}
    for t, x in zip(present, ws):
        row[pos[t]] = np.float32(x / tot)
    return row, True


def _mask_identity(mask) -> Optional[tuple]:
    return None if mask is None else (mask.data_ptr(), mask.numel(), str(mask.device), mask.dtype)


def _source_walk_decline(batch, noise_batch, name, mask) -> Optional[str]:
    """Why a masked parameter of a fused run cannot take the source-walk consumers (svdq_merge_masked,
    svdq_task_reconstruct_masked), or None when it can: they put the rows back with the mask table and unit starts the
    run compressed with, so the caller's ``mask`` must be that very tensor -- for the signal batch and, when the
    parameter has a noise entry to merge, for its ``noise_batch`` too."""
    if getattr(batch, "mode", "plain") == "plain":
        return "the batch was not compressed through masks"
    ident = getattr(batch, "mask_ident", {}).get(name)
    if ident is None:
        return "the run recorded no mask for the parameter"
    if ident != _mask_identity(mask):
        return "the caller's mask is not the tensor the run compressed with"
    if batch.unit_start is None:
        return "the batch has no unit starts"
    if noise_batch is not None:
        if noise_batch.unit_start is None:
            return "the noise batch has no unit starts"
        if getattr(noise_batch, "mask_ident", {}).get(name) != ident:
            return "the noise batch was compressed with another mask"
    return None


def _merge_batched(names, compressed_all, bases, masks, sets, original_shapes, config, device):
    """merge_all_parameters / merge_with_clustering for the parameters whose artifacts still live in the buffers of a
    fused run: per plan ONE coefficient kernel + ONE streaming reconstruction (svdq_merge) instead of, per parameter
    and task, a host->device copy of the payloads, a dequantize launch, a stack/sum and a reconstruct launch.  Masked
    parameters: the same two launches per plan with reconstruct_from_masked inside the streaming one
    (svdq_merge_masked: signal and noise regions write their own rows of the full tensor).
    ``sets``: [(weights dict, members or None)] and, for more than one set, their shares (device tensor).
    Returns {name: merged delta} for the names it could take; the rest goes the per-parameter way."""
    import numpy as np
    set_list, shares = sets
    S = len(set_list)
    if S > 8:
        return {}
    dev = resolve_device(device)
    jobs = {}      # id(plan) -> (plan batch, {entry index: (name, region, meta)})
    for name in names:
        got = _batched_entry(name, compressed_all, bases)
        if got is None:
            continue
        batch, i, meta = got
        jobs.setdefault(id(batch.plan), (batch, {}))[1][i] = (name, "masked", meta)
        if config.svd_include_noise and meta["noise"] is not None:
            nb, j = meta["noise"]
            jobs.setdefault(id(nb.plan), (nb, {}))[1][j] = (name, "noise", meta)
    # the per-plan tables, and which (parameter, region) pairs have something to merge
    tables, live = {}, {}
    for key, (batch, entries) in jobs.items():
        plan, small = batch.plan, batch.small
        P, N = plan.P, plan.N
        wt = np.full((P, S, N), -1.0, dtype=np.float32)
        order = np.tile(np.arange(N, dtype=np.int32), (P, 1))
        scale = np.ones(P, dtype=np.float32)
        share_ok = np.zeros((P, S), dtype=bool)
        for i, (name, region, meta) in entries.items():
            tasks_i = batch.task_names[i]
            order[i] = np.argsort(np.array(tasks_i, dtype=object), kind="stable").astype(np.int32)
            for s_, (w, members) in enumerate(set_list):
                wt[i, s_], share_ok[i, s_] = _task_weights(meta["have"], tasks_i, members, w)
            if region == "noise":
                scale[i] = np.float32(config.svd_noise_shrink)
            if int(small.rows[i]) > 0 and share_ok[i].any():
                live.setdefault(name, {})[region] = (key, i)
        tables[key] = (wt, order, scale, share_ok)
    # masked parameters go through the fused scatter when the caller's mask is the one the run compressed with
    full, fused = {}, set()
    for name, regs in live.items():
        if "masked" not in regs:
            continue
        batch = jobs[regs["masked"][0]][0]
        nb = jobs[regs["noise"][0]][0] if "noise" in regs else None
        if _source_walk_decline(batch, nb, name, masks.get(name)) is None:
            fused.add(name)
    pieces = {}    # name -> {"masked": tensor, "noise": tensor} (compacted rows; the unfused way)
    with torch.cuda.device(dev):
        for key, (batch, entries) in jobs.items():
            plan, small = batch.plan, batch.small
            P = plan.P
            wt, order, scale, share_ok = tables[key]
            wt_d = torch.from_numpy(wt).to(plan.device)
            ord_d = torch.from_numpy(order).to(plan.device)
            sc_d = torch.from_numpy(scale).to(plan.device)
            sh_d = None
            if S > 1:
                # merge_with_clustering (merge.py:555-626) merges EVERY parameter inside every cluster -- a cluster none of
                # whose members has it contributes merge_parameter's zeros (merge.py:297-299) -- so
                # apply_weights_to_tensors (weighting.py:332-372) normalises the shares over ALL clusters, and a
                # parameter only some clusters hold comes out scaled by the sum of THEIR shares (its mean included):
                # shares / shares.sum() for the sets that have it, "skip" (-1) for the others -- no renormalisation
                ok = torch.from_numpy(share_ok).to(plan.device)
                sh = shares.to(plan.device).view(S)
                tot = torch.zeros((), dtype=torch.float32, device=plan.device)
                for s_ in range(S):      # w.sum() of <= 8 values, in set order
                    tot = tot + sh[s_]
                sh_d = torch.where(ok, (sh / tot).view(1, S).expand(P, S),
                                   torch.full((), -1.0, device=plan.device)).contiguous()
            rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * P].view(torch.int64)
            mine = {i: e for i, e in entries.items() if live.get(e[0], {}).get(e[1]) == (key, i)}
            take = {i: e for i, e in mine.items() if e[0] in fused}
            if take:
                out_tab = np.zeros(P, dtype=np.int64)
                fill = np.zeros(P, dtype=np.int32)
                for i, (name, region, meta) in take.items():
                    if name not in full:
                        full[name] = torch.empty(plan.rows[i], dtype=torch.float32, device=plan.device)
                    out_tab[i] = full[name].data_ptr()
                    fill[i] = int(region == "masked" and "noise" not in live[name])
                plan.merge_masked(wt_d, batch.mask_table, batch.unit_start, rows_dev,
                                  torch.from_numpy(out_tab).to(plan.device), order=ord_d, set_share=sh_d, scale=sc_d,
                                  fill=torch.from_numpy(fill).to(plan.device))
            if len(take) < len(mine):
                # a buffer of this call's own: the reference returns fresh tensors, and a later merge of the same plan
                # (other weights, an ablation) must not overwrite what this one handed out
                buf, offs, otab = plan.new_merged_outputs()
                plan.merge(wt_d, order=ord_d, set_share=sh_d, scale=sc_d, rows_dev=rows_dev, out_table=otab)
                for i, (name, region, meta) in mine.items():
                    if i not in take:
                        pieces.setdefault(name, {})[region] = buf[offs[i]:offs[i] + int(small.rows[i])]
    from .mask_loader import reconstruct_from_masked
    out = {name: t.view(original_shapes[name]) for name, t in full.items()}
    for name, pc in pieces.items():
        if "masked" not in pc:
            continue
        mask = masks.get(name)
        if mask is not None:
            res = reconstruct_from_masked(pc["masked"], pc.get("noise"), mask, original_shapes[name])
        else:
            res = pc["masked"].view(original_shapes[name])
        out[name] = res
    return out


def merge_all_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                         masks: Dict[str, torch.Tensor], weights: Dict[str, float],
                         original_shapes: Dict[str, torch.Size], config, device: str = "cpu",
                         verbose: bool = True) -> Dict[str, torch.Tensor]:
    """Reference merge.py:304-426: parameters in sorted order, one quantizer for the run."""
    quantizer = RTVQQuantizer(num_bits=config.svd_low_bits, num_stages=config.svd_rtvq_stages)
    names = sorted(compressed_all.keys())
    # parameters whose artifacts still live in a fused run's buffers: two launches per plan (svdq_merge)
    fast = _merge_batched(names, compressed_all, bases, masks, ([(weights, None)], None), original_shapes, config, device)
    merged = {}
    for name in names:
        if name in fast:
            merged[name] = fast[name].cpu() if wants_cpu(device) else fast[name]
            continue
        merged[name] = merge_parameter(name, compressed_all[name], bases[name], weights, quantizer,
                                       original_shapes[name], mask=masks.get(name),
                                       include_noise=config.svd_include_noise, noise_shrink=config.svd_noise_shrink,
                                       device=device)
    if verbose:
        print(f"   merged {len(merged)} parameters")
    return merged


def _task_walk_plans(where, masks, original_shapes, config):
    """``fused_masks``: the masked parameters whose rows go back at their source positions inside the launch
    (svdq_task_reconstruct_masked), and per plan the tables it walks with.  A parameter of a fused run qualifies exactly
    when ``_merge_batched`` sends it through svdq_merge_masked (``_source_walk_decline``); one of adopted plans when the
    caller's mask fits the stored row counts (``driver.adopted_mask_walk``).  Returns ({id(plan): (mask_table,
    unit_start)}, names, names with a live noise entry)."""
    import math
    from .driver import adopted_mask_walk
    walk = {}

    def tables(batch):
        key = id(batch.plan)
        if key not in walk:
            walk[key] = (adopted_mask_walk(batch, masks) if getattr(batch, "adopted", False)
                         else (batch.mask_table, batch.unit_start, None))
        return walk[key]

    def fits(batch, i):      # an adopted entry: the caller's mask selects exactly its stored rows
        t = tables(batch)
        return t is not None and i in t[2]

    fused, noisy = set(), set()
    for name, (batch, i, meta) in where.items():
        mask = masks.get(name)
        if mask is None or int(batch.small.rows[i]) <= 0:
            continue
        if batch.plan.rows[i] != mask.numel() or math.prod(original_shapes[name]) != mask.numel():
            continue
        nb = j = None
        if config.svd_include_noise and meta["noise"] is not None and int(meta["noise"][0].small.rows[meta["noise"][1]]) > 0:
            nb, j = meta["noise"]
            # fill is per parameter: the noise entry must cover every task the signal entry has
            if nb.task_names[j] != batch.task_names[i] or nb.plan.rows[j] != mask.numel():
                continue
        adopted = getattr(batch, "adopted", False)
        if nb is not None and getattr(nb, "adopted", False) != adopted:
            continue
        if adopted:
            ok = fits(batch, i) and (nb is None or fits(nb, j))
        else:
            ok = _source_walk_decline(batch, nb, name, mask) is None
            if ok:
                tables(batch)
                if nb is not None:
                    tables(nb)
        if ok:
            fused.add(name)
            if nb is not None:
                noisy.add(name)
    return {key: t[:2] for key, t in walk.items() if t is not None}, fused, noisy


def _reconstruct_tasks_batched(names, wanted, compressed_all, bases, masks, original_shapes, config, base_state_dict, dev,
                               fused_masks=False):
    """reconstruct_task_vectors for the parameters whose artifacts live in plans (a fused run's, or adopted ones): per
    plan ONE svdq_task_reconstruct -- the selected tasks' coefficients + one pass over the basis that writes every
    (parameter, task) output -- into a buffer of this call's own.  Unmasked parameters get ``base +`` inside the launch;
    masked ones are formed in compacted rows (the noise plan with scale = svd_noise_shrink) and scattered per task
    afterwards -- or, with ``fused_masks``, written at their source rows by ONE svdq_task_reconstruct_masked per plan
    (full tensors of this call's own; fill = 1 on a signal entry without a live noise entry; a fp32 base of the right
    size inside the launch).  Returns {name: {task: tensor}} for the names it could take."""
    import numpy as np
    from .mask_loader import reconstruct_from_masked
    jobs, metas, where = {}, {}, {}      # id(plan) -> (plan batch, {entry index: (name, region)})
    for name in names:
        got = _batched_entry(name, compressed_all, bases)
        if got is None:
            continue
        batch, i, meta = got
        metas[name], where[name] = meta, got
        jobs.setdefault(id(batch.plan), (batch, {}))[1][i] = (name, "masked")
        if config.svd_include_noise and meta["noise"] is not None:
            nb, j = meta["noise"]
            jobs.setdefault(id(nb.plan), (nb, {}))[1][j] = (name, "noise")
    want = set(wanted)
    walk, fused, noisy = _task_walk_plans(where, masks, original_shapes, config) if fused_masks else ({}, set(), set())
    pieces = {}      # name -> task -> {"masked": rows, "noise": rows} (compacted rows where the parameter is masked)
    full, based_in = {}, set()      # name -> task -> full tensor (fused masks); names whose base went inside the launch
    with torch.cuda.device(dev):
        for key, (batch, all_entries) in jobs.items():
            plan, small = batch.plan, batch.small
            P = plan.P
            rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * P].view(torch.int64)
            for walked in (True, False):
                entries = {i: e for i, e in all_entries.items() if (e[0] in fused) == walked}
                # the plan's task positions some entry wants; an entry whose task at a position is not wanted (plans group
                # by task COUNT: two entries may name their tasks differently) leaves that output out
                slots = sorted({q for i, (name, _) in entries.items() for q, t in enumerate(batch.task_names[i])
                                if t in want and t in metas[name]["have"]})
                if not slots:
                    continue
                n_out = len(slots)
                out_tab = np.zeros((P, n_out), dtype=np.int64)
                base_tab = np.zeros(P, dtype=np.int64)
                scale = np.ones(P, dtype=np.float32)
                fill = np.zeros(P, dtype=np.int32)
                cuts, tot, keep = [], 0, []
                for i, (name, region) in entries.items():
                    rows = int(small.rows[i])
                    if rows <= 0:
                        continue
                    if region == "noise":
                        scale[i] = np.float32(config.svd_noise_shrink)
                    b = base_state_dict.get(name) if base_state_dict is not None else None
                    if walked:
                        fill[i] = int(region == "masked" and name not in noisy)
                        if b is not None and b.dtype is torch.float32 and b.numel() == plan.rows[i]:
                            keep.append(prepare_vector(b, plan.device))
                            base_tab[i] = keep[-1].data_ptr()
                            based_in.add(name)
                    elif b is not None and masks.get(name) is None and b.dtype is torch.float32 and b.numel() == rows:
                        keep.append(prepare_vector(b, plan.device))
                        base_tab[i] = keep[-1].data_ptr()
                    for j, q in enumerate(slots):
                        t = batch.task_names[i][q]
                        if not (t in want and t in metas[name]["have"]):
                            continue
                        if walked:
                            # full tensors of this call's own; the signal and the noise entry write their own rows of it
                            ft = full.setdefault(name, {}).get(t)
                            if ft is None:
                                ft = full[name][t] = torch.empty(plan.rows[i], dtype=torch.float32, device=plan.device)
                            out_tab[i, j] = ft.data_ptr()
                        else:
                            cuts.append((i, j, name, region, t, tot, rows, bool(base_tab[i])))
                            tot += (rows + 63) // 64 * 64
                sc_d = torch.from_numpy(scale).to(plan.device)
                bt_d = torch.from_numpy(base_tab).to(plan.device) if base_tab.any() else None
                if walked:
                    if not out_tab.any():      # only entries without rows (a noise region that was not built)
                        continue
                    mask_table, unit_start = walk[key]
                    plan.reconstruct_tasks_masked(slots, mask_table, unit_start, rows_dev,
                                                  torch.from_numpy(out_tab).to(plan.device), scale=sc_d,
                                                  fill=torch.from_numpy(fill).to(plan.device), base_table=bt_d)
                    continue
                # a buffer of this call's own: a later call must not overwrite what this one hands out
                buf = torch.empty(tot, dtype=torch.float32, device=plan.device)
                for i, j, _, _, _, off, _, _ in cuts:
                    out_tab[i, j] = buf.data_ptr() + 4 * off
                plan.reconstruct_tasks(slots, torch.from_numpy(out_tab).to(plan.device), scale=sc_d, base_table=bt_d,
                                       rows_dev=rows_dev)
                for _, _, name, region, t, off, rows, based in cuts:
                    pieces.setdefault(name, {}).setdefault(t, {})[region] = (buf[off:off + rows], based)
        out = {}
        for name, meta in metas.items():
            shape, mask = original_shapes[name], masks.get(name)
            b = base_state_dict.get(name) if base_state_dict is not None else None
            res = {}
            for t in meta["have"]:
                if t not in want:
                    continue
                pc = pieces.get(name, {}).get(t, {})
                based = False
                if name in fused and t in full.get(name, {}):
                    delta, based = full[name][t].view(shape), name in based_in
                elif "masked" not in pc:
                    delta = torch.zeros(shape, device=dev)      # merge_parameter's zeros (merge.py:297-299)
                elif mask is not None:
                    delta = reconstruct_from_masked(pc["masked"][0], pc["noise"][0] if "noise" in pc else None, mask, shape)
                else:
                    delta, based = pc["masked"][0].view(shape), pc["masked"][1]
                res[t] = delta if (b is None or based) else b.to(delta.device) + delta
            out[name] = res
    return out


def reconstruct_task_vectors(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                             masks: Optional[Dict[str, torch.Tensor]], original_shapes: Dict[str, torch.Size], config,
                             tasks=None, device: str = "cpu", base_state_dict: Optional[Dict[str, torch.Tensor]] = None
                             ) -> Dict[str, Dict[str, torch.Tensor]]:
    """Every task's own task vector back out of the artifacts: {task: {param: U c_task + mean}}, what the reference
    computes per (parameter, task) with RTVQQuantizer.dequantize (rtvq.py:85-103) + reconstruct_from_coefficients
    (merge.py:144-194) -- here ``merge_parameter`` on that task alone with weight 1.0, bit for bit.  ``tasks``: the task
    names wanted (None = every task of ``compressed_all``).  ``base_state_dict``: the values are ``base + delta`` for the
    parameters it holds (apply_merged_deltas, merge.py:429-552).  A task that lacks a parameter has no such key.

    Parameters whose dictionaries still are what a fused run or ``adopt_artifacts`` handed out take two launches per
    plan for ALL selected tasks (svdq_task_reconstruct: one pass over the basis, n outputs); the rest goes per
    (parameter, task) through ``merge_parameter``.  Masked parameters of such plans are formed in compacted rows and put
    back per (parameter, task); ``reconstruct_task_vectors_masked`` does that inside the streaming launch."""
    return reconstruct_task_vectors_masked(compressed_all, bases, masks, original_shapes, config, tasks=tasks,
                                           device=device, base_state_dict=base_state_dict, fused_masks=False)


def reconstruct_task_vectors_masked(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                                    masks: Optional[Dict[str, torch.Tensor]], original_shapes: Dict[str, torch.Size],
                                    config, tasks=None, device: str = "cpu",
                                    base_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                                    fused_masks: bool = True) -> Dict[str, Dict[str, torch.Tensor]]:
    """``reconstruct_task_vectors`` for masked runs: the same arguments, the same result bit for bit, and one keyword.
    (A function of its own because the signature of ``reconstruct_task_vectors`` is part of the surface this package
    holds fixed; that function is this one with ``fused_masks=False``.)

    ``fused_masks``: masked parameters of such plans get reconstruct_from_masked (mask_loader.py:712-763) and ``base +``
    INSIDE the streaming launch (svdq_task_reconstruct_masked) instead of compacted rows scattered per (parameter,
    task) afterwards -- when ``masks[name]`` is the tensor the run compressed with, or, for adopted plans
    (``adopt_artifacts(..., masks=masks)``), a mask that selects exactly the stored rows; any other masked parameter
    keeps the compacted route.  Same bits either way."""
    wanted = None if tasks is None else list(tasks)      # the caller's order, repeats included
    known, _ = _store_tasks(compressed_all, wanted)
    wanted = list(known) if wanted is None else wanted
    dev = resolve_device(device)
    masks = masks or {}
    quantizer = RTVQQuantizer(num_bits=config.svd_low_bits, num_stages=config.svd_rtvq_stages)
    names = sorted(compressed_all.keys())
    fast = _reconstruct_tasks_batched(names, wanted, compressed_all, bases, masks, original_shapes, config,
                                      base_state_dict, dev, fused_masks=fused_masks)
    out = {t: {} for t in wanted}
    for name in names:
        if name in fast:
            per = fast[name]
        else:
            per = {}
            b = base_state_dict.get(name) if base_state_dict is not None else None
            for t in wanted:
                if t not in compressed_all[name]:
                    continue
                delta = merge_parameter(name, {t: compressed_all[name][t]}, bases[name], {t: 1.0}, quantizer,
                                        original_shapes[name], mask=masks.get(name),
                                        include_noise=config.svd_include_noise, noise_shrink=config.svd_noise_shrink,
                                        device=dev)
                per[t] = delta if b is None else b.to(delta.device) + delta
        for t in wanted:
            if t in per:
                out[t][name] = per[t].cpu() if wants_cpu(device) else per[t]
    return out


def apply_merged_deltas(base_state_dict: Dict[str, torch.Tensor], merged_deltas: Dict[str, torch.Tensor],
                        device: str = "cpu", verbose: bool = True) -> Dict[str, torch.Tensor]:
    """Reference merge.py:429-552: merged[param] = base[param] + delta[param]; others are cloned."""
    out = {}
    for name, base in base_state_dict.items():
        if name in merged_deltas:
            out[name] = base + merged_deltas[name].to(base.device)
        else:
            out[name] = base.clone()
    if verbose:
        print(f"   applied {sum(n in merged_deltas for n in base_state_dict)} merged deltas")
    return out


def _merge_with_clustering_batched(compressed_all, bases, masks, weights, clusters, original_shapes, config, device):
    """merge_with_clustering when EVERY parameter can take the batched route: the per-cluster merges and the share-weighted
    sum over clusters happen inside one streaming pass per plan (the merge is linear in the coefficients).  None
    otherwise (then the per-cluster loop below runs)."""
    names = sorted(compressed_all.keys())
    if not names or len(clusters) > 8 or any(_batched_entry(n, compressed_all, bases) is None for n in names):
        return None
    cids = sorted(clusters.keys())      # apply_weights_to_tensors adds the clusters in sorted-key order
    sets, perf = [], []
    for cid in cids:
        members = clusters[cid]
        w = {m: weights.get(m, 1.0) for m in members}
        total = sum(w.values())
        sets.append(({m: v / total for m, v in w.items()}, set(members)))
        perf.append(sum(weights.get(m, 1.0) for m in members) / len(members))
    # clustering.merge_cluster_results: softmax over the clusters in their first-seen order, looked up per cluster id
    seen = list(clusters.keys())
    sm = torch.softmax(torch.tensor([perf[cids.index(c)] for c in seen]), dim=0)
    by_cid = {c: sm[j].item() for j, c in enumerate(seen)}
    dev = resolve_device(device)
    shares = torch.tensor([by_cid[c] for c in cids], device=dev, dtype=torch.float32)
    fast = _merge_batched(names, compressed_all, bases, masks, (sets, shares), original_shapes, config, device)
    if len(fast) != len(names):
        return None
    return {n: (t.cpu() if wants_cpu(device) else t) for n, t in fast.items()}


def merge_with_clustering(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                          masks: Dict[str, torch.Tensor], weights: Dict[str, float],
                          cluster_assignments: Dict[str, int], original_shapes: Dict[str, torch.Size], config,
                          device: str = "cpu") -> Dict[str, torch.Tensor]:
    """Reference merge.py:555-626: merge inside each cluster (weights renormalised over its members), then
    average the cluster results with softmax(mean member weight) shares (clustering.py:374-425)."""
    from .clustering import get_cluster_members, merge_cluster_results
    clusters = get_cluster_members(cluster_assignments)
    fast = _merge_with_clustering_batched(compressed_all, bases, masks, weights, clusters, original_shapes, config, device)
    if fast is not None:
        return fast
    per_cluster, performance = {}, {}
    for cid, members in clusters.items():
        w = {m: weights.get(m, 1.0) for m in members}
        total = sum(w.values())
        w = {m: v / total for m, v in w.items()}
        subset = {p: {m: arts[m] for m in members if m in arts} for p, arts in compressed_all.items()}
        per_cluster[cid] = merge_all_parameters(subset, bases, masks, w, original_shapes, config, device,
                                                verbose=False)
        performance[cid] = sum(weights.get(m, 1.0) for m in members) / len(members)
    return merge_cluster_results(per_cluster, performance, device)


def _store_tasks(compressed_all, tasks, who=None):
    """(known, wanted): the task names of a store in first-seen order, and -- for the merge ``who`` -- the names it
    merges: ``tasks`` (None = all) distinct and sorted, between 1 and MAX_TASKS of them.  ``who=None``: no merge,
    ``wanted`` is None.  A name of ``tasks`` the store lacks raises the ValueError that lists what it holds."""
    known = []
    for per_task in compressed_all.values():
        known += [t for t in (per_task._meta["have"] if getattr(per_task, "_meta", None) else per_task.keys())
                  if t not in known]
    for t in (tasks if tasks is not None else []):
        if t not in known:
            raise ValueError(f"unknown task {t!r}: the artifacts hold {known}")
    if who is None:
        return known, None
    wanted = sorted(set(known if tasks is None else tasks))
    if not 1 <= len(wanted) <= nat.MAX_TASKS:
        raise ValueError(f"{who}: between 1 and {nat.MAX_TASKS} tasks can be merged, got {len(wanted)}")
    return known, wanted


def _is_number(x, nonneg: bool = False) -> bool:
    """A finite int or float, no bool; with ``nonneg`` also >= 0."""
    import math
    return (not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x) and not (nonneg and x < 0))


def _as_fp32(values):
    """(``values`` rounded to a float32 array, whether every entry stayed finite)."""
    import numpy as np
    with np.errstate(over="ignore"):
        v32 = np.asarray(values, dtype=np.float64).astype(np.float32)
    return v32, bool(np.isfinite(v32).all())


def _slot_tables(P, entries, live, offsets=None):
    """The host tables of one plan for a pass over every task's own values (pure numpy): slot_task [P][n_out] the plan
    task of every slot, task_map [P][n_out] its store task (-1 = the slot is empty) -- per parameter the pairs of
    ``live`` (``_ties_jobs``) in store order, n_out the most any parameter of ``entries`` has, at least 1 -- and an
    int64 column [P] of ``offsets[name]`` (0 without: DARE's first global row, the first bit of a mask stream)."""
    import numpy as np
    n_out = max([len(live[name]) for name in entries.values()] + [1])
    slot_task = np.zeros((P, n_out), dtype=np.int32)
    task_map = np.full((P, n_out), -1, dtype=np.int32)
    column = np.zeros(P, dtype=np.int64)
    for i, name in entries.items():
        for j, (g, q) in enumerate(live[name]):
            task_map[i, j], slot_task[i, j] = g, q
        if offsets is not None:
            column[i] = offsets.get(name, 0)
    return slot_task, task_map, column


def _stage_base(name, count, base_state_dict, device, keep, later) -> int:
    """The address of ``base_state_dict[name]`` for a launch to add: a fp32 base of ``count`` elements, made a contiguous
    device vector that ``keep`` holds.  0 without a base, and for any other base -- that one goes to ``later``, to be
    added to the result in its own arithmetic (``_finish_output``)."""
    b = base_state_dict.get(name) if base_state_dict is not None else None
    if b is not None and b.dtype is torch.float32 and b.numel() == count:
        keep.append(prepare_vector(b, device))
        return keep[-1].data_ptr()
    if b is not None:
        later[name] = b
    return 0


def _plan_outputs(plan, entries, rows, original_shapes, base_state_dict, out, later):
    """The device side of one plan's launch: a fresh fp32 output per parameter of ``entries`` into ``out`` (zeros in its
    shape for a parameter without rows; ``out=None``: no outputs at all), the bases staged (``_stage_base``).  Returns
    (out_tab or None, base_tab or None, rows_dev, the tensors the launch needs kept alive)."""
    import numpy as np
    P = plan.P
    rows_dev = plan.small[plan.layout.rows_off:plan.layout.rows_off + 8 * P].view(torch.int64)
    if out is None:
        return None, None, rows_dev, []
    out_tab = np.zeros(P, dtype=np.int64)
    base_tab = np.zeros(P, dtype=np.int64)
    keep = []
    for i, name in entries.items():
        if rows[name] <= 0:
            out[name] = torch.zeros(original_shapes[name], device=plan.device)
            continue
        res = out[name] = torch.empty(rows[name], dtype=torch.float32, device=plan.device)
        out_tab[i] = res.data_ptr()
        base_tab[i] = _stage_base(name, rows[name], base_state_dict, plan.device, keep, later)
    return (torch.from_numpy(out_tab).to(plan.device),
            torch.from_numpy(base_tab).to(plan.device) if base_tab.any() else None, rows_dev, keep)


def _finish_output(res, shape, name, later, device):
    """A launch's flat output as the caller gets it: in ``shape``, plus the base that could not go into the launch, on
    the CPU when ``device`` asks for it."""
    res = res.view(shape)
    if name in later:
        res = later[name].to(res.device) + res
    return res.cpu() if wants_cpu(device) else res


def _ties_jobs(names, wanted, compressed_all, bases, original_shapes, who="ties_merge_parameters", what="the TIES merge"):
    """The plans behind a TIES (or DARE: ``who`` / ``what`` name the caller in the messages) merge: {id(plan): (batch,
    {entry index: name})}, the rows of every parameter and, per parameter, the (store task, plan task) pairs of the
    wanted tasks that have it, in store order.  Raises the named ValueError for what the streaming route cannot serve."""
    import math
    jobs, rows, live = {}, {}, {}
    for name in names:
        got = _batched_entry(name, compressed_all, bases)
        if got is None:
            raise ValueError(f"{who}: parameter {name!r} is not backed by a plan (adoption declined it, or "
                             f"its dictionaries were edited): {what} reads the values from plans only")
        batch, i, meta = got
        stored = int(batch.small.rows[i])
        if (getattr(batch, "mode", "plain") != "plain" or meta["noise"] is not None
                or stored != math.prod(original_shapes[name])):
            raise ValueError(f"{who}: parameter {name!r} stores {stored} rows for a tensor of "
                             f"{math.prod(original_shapes[name])} elements -- a masked run's store; masks are not stored, "
                             f"and {what} is defined on whole tensors")
        jobs.setdefault(id(batch.plan), (batch, {}))[1][i] = name
        rows[name] = stored
        pos = {t: q for q, t in enumerate(batch.task_names[i])}
        live[name] = [(g, pos[t]) for g, t in enumerate(wanted) if t in meta["have"] and t in pos]
    return jobs, rows, live


def ties_merge_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                          original_shapes: Dict[str, torch.Size], config, density: float = 0.2, scaling: float = 1.0,
                          merge_func: str = "mean", tasks=None, base_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                          device: str = "cuda", return_stats: bool = False):
    """The sign-elected (TIES, Yadav et al. 2023) merge of what a store reconstructs, without a task model ever being
    written (the contract is at svdq_plan_ties_hist in include/svdq.h).  With v_t what
    ``reconstruct_task_vectors`` returns for task t (0 where a task lacks a parameter), D the rows of all parameters and
    the tasks in sorted-name order: trim every task to the values with |v_t| >= tau_t, the j-th smallest magnitude over
    all D rows, j = max(D - int(D * density), 1); elect the sign of the fp32 sum of the kept values per row (>= 0 is
    positive); average (``merge_func="mean"``) or add ("sum") the kept values that agree with it; return
    ``scaling * merged`` per parameter, ``base + scaling * merged`` for the parameters ``base_state_dict`` holds.

    Takes dictionaries backed by a fused run or by ``adopt_artifacts``; ``tasks``: the names to merge (None = all).  A
    parameter that no plan backs, or whose stored rows differ from its shape's element count (a masked run's store),
    raises a ValueError naming it.  ``config`` is the run's (the dictionaries carry everything the merge needs; it is
    taken for symmetry with ``merge_all_parameters``).

    Returns {param: tensor}; with ``return_stats`` also {"thresholds": {task: float}, "kept": {task: int},
    "sign_conflict_rows": int, "empty_rows": int, "rows": D}.  4 passes over the basis find the thresholds exactly, one
    more merges: the only buffers that grow with the model are the outputs."""
    import numpy as np
    from .pipeline import ties_thresholds
    if not (isinstance(density, (int, float)) and 0.0 < float(density) <= 1.0):
        raise ValueError(f"density must be in (0, 1], got {density!r}")
    if merge_func not in ("mean", "sum"):
        raise ValueError(f"merge_func must be 'mean' or 'sum', got {merge_func!r}")
    _, wanted = _store_tasks(compressed_all, tasks, "ties_merge_parameters")
    T = len(wanted)
    names = sorted(compressed_all.keys())
    jobs, rows, live = _ties_jobs(names, wanted, compressed_all, bases, original_shapes)      # refusals before device work
    dev = resolve_device(device)
    D = sum(rows.values())
    rank = max(D - int(D * float(density)), 1)
    zeros = np.full(T, D, dtype=np.int64)
    for name, pairs in live.items():
        for g, _ in pairs:
            zeros[g] -= rows[name]
    out, later = {}, {}
    stats = {"thresholds": {}, "kept": {}, "sign_conflict_rows": 0, "empty_rows": 0, "rows": D}
    if D == 0:
        out = {name: torch.zeros(original_shapes[name], device=dev) for name in names}
        return (out, stats) if return_stats else out
    with torch.cuda.device(dev):
        calls, keep = [], []
        for batch, entries in jobs.values():
            plan = batch.plan
            slot_task, task_map, _ = _slot_tables(plan.P, entries, live)
            out_tab, base_tab, rows_dev, kept = _plan_outputs(plan, entries, rows, original_shapes, base_state_dict, out,
                                                              later)
            keep += kept
            calls.append((plan, torch.from_numpy(slot_task).to(plan.device), torch.from_numpy(task_map).to(plan.device),
                          rows_dev, out_tab, base_tab))
        state = ties_thresholds([c[:4] for c in calls], T, rank, torch.from_numpy(zeros).to(dev), device=dev)
        for plan, slot_task, task_map, rows_dev, out_tab, base_tab in calls:
            plan.ties_merge(slot_task, task_map, T, state.table, out_tab, merge_func=merge_func, scaling=scaling,
                            base_table=base_tab, rows_dev=rows_dev)
        if return_stats:
            host = state.table[256 * T:].cpu().numpy()
            tau = (host[:T] & 0xffffffff).astype(np.uint32).view(np.float32)
            stats["thresholds"] = {t: float(tau[g]) for g, t in enumerate(wanted)}
            stats["kept"] = {t: int(host[2 * T + g]) for g, t in enumerate(wanted)}
            stats["sign_conflict_rows"], stats["empty_rows"] = int(host[3 * T]), int(host[3 * T + 1])
        for name in names:
            out[name] = _finish_output(out[name], original_shapes[name], name, later, device)
    return (out, stats) if return_stats else out


def _crumbs_arguments(density, gamma, scaling, merge_func):
    """The named ValueError for what lies outside the Breadcrumbs definition; (density, gamma) as floats."""
    if not _is_number(density) or not 0.0 < float(density) <= 1.0:
        raise ValueError(f"density must be in (0, 1], got {density!r}")
    if not _is_number(gamma) or not 0.0 <= float(gamma) < 1.0:
        raise ValueError(f"gamma must be in [0, 1), got {gamma!r}")
    if not _is_number(scaling):
        raise ValueError(f"scaling must be a finite number, got {scaling!r}")
    if merge_func not in ("mean", "sum"):
        raise ValueError(f"merge_func must be 'mean' or 'sum', got {merge_func!r}")
    return float(density), float(gamma)


def crumbs_ranks(rows: int, density: float, gamma: float):
    """(rank of lo, rank of hi), 1-based from below among the ``rows`` magnitudes of one (parameter, task); (0, 0) when
    nothing is kept.  Python integers: n_keep = int(D * density), n_top = int(D * gamma), n_bot = D - n_keep - n_top, the
    outlier cut giving way (n_top += n_bot) where n_bot < 0."""
    D = int(rows)
    n_keep, n_top = int(D * density), int(D * gamma)
    n_bot = D - n_keep - n_top
    if n_bot < 0:
        n_top, n_bot = n_top + n_bot, 0
    return (n_bot + 1, D - n_top) if n_keep > 0 else (0, 0)


def breadcrumbs_merge_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                                 original_shapes: Dict[str, torch.Size], config, density: float = 0.9,
                                 gamma: float = 0.01, scaling: float = 1.0, sign_election: bool = False,
                                 merge_func: str = "sum", tasks=None,
                                 base_state_dict: Optional[Dict[str, torch.Tensor]] = None, device: str = "cuda",
                                 return_stats: bool = False):
    """The Model Breadcrumbs merge (Davari & Belilovsky 2023) of what a store reconstructs, and the per-tensor trim,
    without a task model ever being written (the contract is at svdq_plan_crumbs_hist in
    include/svdq.h).  With v_t what ``reconstruct_task_vectors`` returns for task t and the tasks in sorted-name order,
    per parameter of D_p rows and per task that has it: n_keep = int(D_p * density), n_top = int(D_p * gamma), n_bot =
    D_p - n_keep - n_top (where negative, n_top gives way); the value is kept iff lo <= |v| <= hi, lo the (n_bot + 1)-th
    and hi the (D_p - n_top)-th smallest magnitude of that tensor and task (ties at either are all kept; nothing is kept
    where n_keep == 0; ``density=1`` keeps everything).  The kept values are added in task order (``merge_func="sum"``)
    or averaged ("mean"); with ``sign_election`` only those whose sign agrees with the sign of their fp32 sum (>= 0 is
    positive).  Returns ``scaling * merged`` per parameter, ``base + scaling * merged`` for the parameters
    ``base_state_dict`` holds.  A task that lacks a parameter contributes nothing to it.

    The paper's method: ``sign_election=False, merge_func="sum"``, ``density = gamma_paper - beta_paper``, ``gamma = 1 -
    gamma_paper``.  The per-tensor TIES trim: ``gamma=0, sign_election=True, merge_func="mean"``.

    Takes dictionaries backed by a fused run or by ``adopt_artifacts`` and refuses what ``ties_merge_parameters``
    refuses, under its own name; ``tasks``: the names to merge (None = all).  ``density`` outside (0, 1], ``gamma``
    outside [0, 1), a ``scaling`` that is not finite or another ``merge_func`` raises a ValueError.

    Returns {param: tensor}; with ``return_stats`` also {"rows": D, "thresholds": {param: {task: (lo, hi) or None}},
    "kept": {param: {task: int}}, "kept_total": {task: int}, "sign_conflict_rows": int, "empty_rows": int}.  Per plan 4
    digits of histogram passes find both thresholds of every (parameter, task) exactly, one more pass merges: the only
    buffers that grow with the model are the outputs.  The same arguments give the same bits on every call."""
    import numpy as np
    from .pipeline import crumbs_thresholds
    who = "breadcrumbs_merge_parameters"
    density, gamma = _crumbs_arguments(density, gamma, scaling, merge_func)
    _, wanted = _store_tasks(compressed_all, tasks, who)
    T = len(wanted)
    names = sorted(compressed_all.keys())
    jobs, rows, live = _ties_jobs(names, wanted, compressed_all, bases, original_shapes, who,
                                  "the Breadcrumbs merge")      # refusals before device work
    dev = resolve_device(device)
    D = sum(rows.values())
    out, later = {}, {}
    stats = {"rows": D, "thresholds": {}, "kept": {}, "kept_total": {t: 0 for t in wanted}, "sign_conflict_rows": 0,
             "empty_rows": 0}
    if D == 0:
        out = {name: torch.zeros(original_shapes[name], device=dev) for name in names}
        return (out, stats) if return_stats else out
    with torch.cuda.device(dev):
        keep, states = [], []
        for batch, entries in jobs.values():
            plan = batch.plan
            slot_task, task_map, _ = _slot_tables(plan.P, entries, live)
            out_tab, base_tab, rows_dev, kept = _plan_outputs(plan, entries, rows, original_shapes, base_state_dict, out,
                                                              later)
            keep += kept
            ranks = np.zeros((plan.P, 2), dtype=np.int64)
            for i, name in entries.items():
                ranks[i] = crumbs_ranks(rows[name], density, gamma)
            slot_task, task_map = torch.from_numpy(slot_task).to(plan.device), torch.from_numpy(task_map).to(plan.device)
            state = crumbs_thresholds(plan, slot_task, task_map, T, torch.from_numpy(ranks).to(plan.device),
                                      rows_dev=rows_dev)
            plan.crumbs_merge(slot_task, task_map, T, state.table, out_tab, sign_election=sign_election,
                              merge_func=merge_func, scaling=scaling, base_table=base_tab, rows_dev=rows_dev)
            states.append((state, entries))
        if return_stats:
            for state, entries in states:
                P = state.n_params
                host = state.results.cpu().numpy()
                band = (host[:2 * P * T] & 0xffffffff).astype(np.uint32).reshape(P, 2, T)
                band_f = band.view(np.float32)
                kept_pt = host[4 * P * T:5 * P * T].reshape(P, T)
                stats["sign_conflict_rows"] += int(host[5 * P * T])
                stats["empty_rows"] += int(host[5 * P * T + 1])
                for i, name in entries.items():
                    th, kp = stats["thresholds"].setdefault(name, {}), stats["kept"].setdefault(name, {})
                    for g, _ in live[name]:
                        t = wanted[g]
                        nothing = band[i, 0, g] > band[i, 1, g]      # the sentinel band
                        th[t] = None if nothing else (float(band_f[i, 0, g]), float(band_f[i, 1, g]))
                        kp[t] = int(kept_pt[i, g])
                        stats["kept_total"][t] += kp[t]
        for name in names:
            out[name] = _finish_output(out[name], original_shapes[name], name, later, device)
    return (out, stats) if return_stats else out


def _dare_arguments(drop_rate, seed):
    """(drop threshold, q = float32(1 - drop_rate)) of a DARE merge; the named ValueError for what lies outside the
    definition.  Host arithmetic in double: thr = min(int(drop_rate * 2^32), 2^32 - 1); dropped iff word < thr."""
    import math
    import numpy as np
    if (isinstance(drop_rate, bool) or not isinstance(drop_rate, (int, float)) or not math.isfinite(drop_rate)
            or not 0.0 <= float(drop_rate) < 1.0):
        raise ValueError(f"drop_rate must be in [0, 1), got {drop_rate!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    thr = min(int(float(drop_rate) * 2.0 ** 32), 2 ** 32 - 1)
    return thr, float(np.float32(1.0 - float(drop_rate)))


def dare_merge_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                          original_shapes: Dict[str, torch.Size], config, drop_rate: float = 0.9, seed: int = 0,
                          rescale: bool = True, weights=None, normalize: bool = False, scaling: float = 1.0, tasks=None,
                          base_state_dict: Optional[Dict[str, torch.Tensor]] = None, device: str = "cuda",
                          return_stats: bool = False):
    """The drop-and-rescale (DARE, Yu et al. 2024) merge of what a store reconstructs -- and, with ``drop_rate=0``, plain
    task arithmetic from a store -- in one pass over the basis, without a task model ever being written (DESIGN.md
    section 28; the contract is at svdq_plan_dare_merge in include/svdq.h).  With v_t what ``reconstruct_task_vectors``
    returns for task t, the tasks and the parameters in sorted-name order, G the global row (the rows of the parameters
    before it + the row inside the parameter) and g the task's index: the value is dropped iff word ``g & 3`` of
    Philox4x32-10 with key ``seed`` and counter (G, g >> 2) is below ``min(int(drop_rate * 2^32), 2^32 - 1)``; a kept value
    becomes ``v / float32(1 - drop_rate)`` (``rescale=False``: stays v); ``m = m + w_g * x`` over the kept tasks in
    ascending g; the result is ``scaling * m`` per parameter, ``base + scaling * m`` for the parameters
    ``base_state_dict`` holds.  A task that lacks a parameter contributes nothing on its rows.

    ``weights``: None (1.0 for every task: task arithmetic) or {task: number} naming every merged task;
    ``normalize=True`` divides them by their sum (on the host, in double, before rounding to fp32).  ``tasks``: the names
    to merge (None = all).  Takes dictionaries backed by a fused run or by ``adopt_artifacts`` and refuses what
    ``ties_merge_parameters`` refuses, under its own name.  ``drop_rate`` outside [0, 1), a ``seed`` outside [0, 2^64) or
    a weight that is missing or not finite raises a ValueError.  Outputs are fp32.

    Returns {param: tensor}; with ``return_stats`` also {"kept": {task: int}, "rows": D, "drop_threshold": thr}.  The
    same arguments give the same bits on every call."""
    import math
    import numpy as np
    who = "dare_merge_parameters"
    thr, q = _dare_arguments(drop_rate, seed)
    _, wanted = _store_tasks(compressed_all, tasks, who)
    T = len(wanted)
    if weights is None:
        w64 = [1.0] * T
    else:
        if not hasattr(weights, "get"):
            raise ValueError(f"{who}: weights must be None or a mapping {{task: number}}, got {type(weights).__name__}")
        w64 = []
        for t in wanted:
            w = weights.get(t)
            if w is None:
                raise ValueError(f"{who}: the weight of task {t!r} is missing")
            if not _is_number(w):
                raise ValueError(f"{who}: the weight of task {t!r} is not a finite number: {w!r}")
            w64.append(float(w))
    if normalize:
        total = math.fsum(w64)
        if not (math.isfinite(total) and total != 0.0):
            raise ValueError(f"{who}: normalize=True needs weights with a non-zero sum, got {total!r}")
        w64 = [w / total for w in w64]
    w32, ok = _as_fp32(w64)
    if not ok:
        raise ValueError(f"{who}: a weight is not finite in fp32: {w32.tolist()}")
    names = sorted(compressed_all.keys())
    jobs, rows, live = _ties_jobs(names, wanted, compressed_all, bases, original_shapes, who,
                                  "the DARE merge")      # refusals before device work
    dev = resolve_device(device)
    D = sum(rows.values())
    row_base, at = {}, 0
    for name in names:
        row_base[name] = at
        at += rows[name]
    out, later = {}, {}
    stats = {"kept": {t: 0 for t in wanted}, "rows": D, "drop_threshold": thr}
    if D == 0:
        out = {name: torch.zeros(original_shapes[name], device=dev) for name in names}
        return (out, stats) if return_stats else out
    with torch.cuda.device(dev):
        need = int(nat.lib().svdq_dare_work_bytes(T))
        state = torch.zeros(need // 8, dtype=torch.int64, device=dev)
        w_dev = torch.from_numpy(w32).to(dev)
        keep = []
        for batch, entries in jobs.values():
            plan = batch.plan
            slot_task, task_map, base_rows = _slot_tables(plan.P, entries, live, row_base)
            out_tab, base_tab, rows_dev, kept = _plan_outputs(plan, entries, rows, original_shapes, base_state_dict, out,
                                                              later)
            keep += kept
            plan.dare_merge(torch.from_numpy(slot_task).to(plan.device), torch.from_numpy(task_map).to(plan.device), T,
                            torch.from_numpy(base_rows).to(plan.device), w_dev, state, out_tab, seed=seed,
                            drop_threshold=thr, keep_scale=q if rescale else 0.0, scaling=scaling, base_table=base_tab,
                            rows_dev=rows_dev)
        if return_stats:
            host = state.cpu().numpy()
            stats["kept"] = {t: int(host[g]) for g, t in enumerate(wanted)}
        for name in names:
            out[name] = _finish_output(out[name], original_shapes[name], name, later, device)
    return (out, stats) if return_stats else out


def _tall_arguments(who, tall_lambda, k, wanted, check_k=True):
    """(float32 lambdas [T] in the order of ``wanted``, k) of a TALL / consensus call; the named ValueError for what lies
    outside the definition: a lambda that is no finite number >= 0 (in fp32), a mapping that misses a merged task, a k
    that is no integer in [0, T] (``check_k=False``: masks only, k is not looked at)."""
    T = len(wanted)

    def number(x, what):
        if not _is_number(x, nonneg=True):
            raise ValueError(f"{who}: {what} must be a finite number >= 0, got {x!r}")
        return float(x)
    if hasattr(tall_lambda, "get"):
        lam = []
        for t in wanted:
            if tall_lambda.get(t) is None:
                raise ValueError(f"{who}: the tall_lambda of task {t!r} is missing")
            lam.append(number(tall_lambda.get(t), f"the tall_lambda of task {t!r}"))
    else:
        lam = [number(tall_lambda, "tall_lambda")] * T
    lam32, ok = _as_fp32(lam)
    if not ok:
        raise ValueError(f"{who}: a tall_lambda is not finite in fp32: {lam32.tolist()}")
    if check_k and (isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= T):
        raise ValueError(f"{who}: k must be an integer in [0, {T}] (the merged tasks), got {k!r}")
    return lam32, k


def _tall_run(who, compressed_all, bases, original_shapes, tall_lambda, k, scaling, tasks, base_state_dict,
              reference_state_dict, remove_keys, want_merge, want_masks, device):
    """The launches behind ``consensus_merge_parameters`` and ``tall_masks_from_store``: (merged or None, masks or None,
    stats).  Every refusal is raised before device work."""
    _, wanted = _store_tasks(compressed_all, tasks, who)
    T = len(wanted)
    lam32, k = _tall_arguments(who, tall_lambda, k, wanted, check_k=want_merge)
    names = sorted(compressed_all.keys())
    jobs, rows, live = _ties_jobs(names, wanted, compressed_all, bases, original_shapes, who,
                                  "the consensus merge" if want_merge else "the TALL mask")      # before device work
    bit_base, total_bits = (_mask_stream_layout(who, names, rows, reference_state_dict, remove_keys) if want_masks
                            else ({}, 0))
    dev = resolve_device(device)
    D = sum(rows.values())
    out, later = ({}, {}) if want_merge else (None, {})
    stats = {"active": {t: 0 for t in wanted}, "agreement": [D] + [0] * T, "rows": D}
    with torch.cuda.device(dev):
        streams, mask_tab = _new_mask_streams(T, total_bits, dev) if want_masks else (None, None)
        if D > 0:
            need = int(nat.lib().svdq_tall_work_bytes(T))
            state = torch.zeros(need // 8, dtype=torch.int64, device=dev)
            lam_dev = torch.from_numpy(lam32).to(dev)
            keep = []
            for batch, entries in jobs.values():
                plan = batch.plan
                slot_task, task_map, bits = _slot_tables(plan.P, entries, live, bit_base)
                out_tab, base_tab, rows_dev, kept = _plan_outputs(plan, entries, rows, original_shapes, base_state_dict,
                                                                  out, later)
                keep += kept
                plan.tall_consensus(torch.from_numpy(slot_task).to(plan.device), torch.from_numpy(task_map).to(plan.device),
                                    T, torch.from_numpy(bits).to(plan.device), lam_dev, state, out_table=out_tab,
                                    mask_table=mask_tab, min_agree=k if want_merge else 0, scaling=scaling,
                                    base_table=base_tab, rows_dev=rows_dev)
            host = state.cpu().numpy()
            stats["active"] = {t: int(host[g]) for g, t in enumerate(wanted)}
            stats["agreement"] = [int(x) for x in host[T:2 * T + 1]]
        if want_merge:
            for name in names:
                if D == 0:
                    out[name] = torch.zeros(original_shapes[name], device=dev)
                out[name] = _finish_output(out[name], original_shapes[name], name, later, device)
        masks = _packed_masks(streams, wanted, total_bits, device) if want_masks else None
    return out, masks, stats


def consensus_merge_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                               original_shapes: Dict[str, torch.Size], config, tall_lambda=0.4, k: int = 2,
                               scaling: float = 1.0, tasks=None,
                               base_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                               reference_state_dict: Optional[Dict[str, torch.Tensor]] = None, remove_keys=None,
                               return_masks: bool = False, device: str = "cuda", return_stats: bool = False):
    """TALL masks and the consensus merge (Wang et al. 2024) of what a store reconstructs, in one pass over the basis,
    without a task model ever being written (the contract is at svdq_plan_tall_consensus in
    include/svdq.h).  With v_t what ``reconstruct_task_vectors`` returns for task t and the tasks in sorted-name order:
    S = the fp32 sum of the values task by task; task t's mask is ``|v_t| > lambda_t * |S - v_t|`` (strict); a row is kept
    iff at least ``k`` masks are set there; the result is ``scaling * (kept ? S : 0)`` per parameter,
    ``base + scaling * ...`` for the parameters ``base_state_dict`` holds.  ``k=0`` is task arithmetic.  A task that lacks
    a parameter contributes nothing on its rows, and its mask is 0 there.

    ``tall_lambda``: a number or {task: number} naming every merged task, finite and >= 0; ``k``: an integer in
    [0, merged tasks] -- neither is clamped, a value outside raises a ValueError.  ``tasks``: the names to merge (None =
    all).  Takes dictionaries backed by a fused run or by ``adopt_artifacts`` and refuses what ``dare_merge_parameters``
    refuses, under its own name.  Outputs are fp32.

    ``return_masks`` adds {task: uint8 tensor}: the masks bit-packed as ``numpy.packbits`` packs them, over the sorted
    keys of ``reference_state_dict`` minus ``remove_keys`` (default: the store's own parameters) -- the streams a
    TALL_mask_{T}task file holds.  Keys of the reference that the store lacks occupy zero bits; a store parameter without
    a place in the reference, or with another element count there, raises a ValueError.

    Returns {param: tensor}, then the masks with ``return_masks``, then {"active": {task: set bits}, "agreement": [rows
    with 0 .. T set masks], "rows": D} with ``return_stats``.  The same arguments give the same bits on every call."""
    out, masks, stats = _tall_run("consensus_merge_parameters", compressed_all, bases, original_shapes, tall_lambda, k,
                                  scaling, tasks, base_state_dict, reference_state_dict, remove_keys, True,
                                  bool(return_masks), device)
    res = (out,) + ((masks,) if return_masks else ()) + ((stats,) if return_stats else ())
    return res if len(res) > 1 else out


def tall_masks_from_store(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                          original_shapes: Dict[str, torch.Size], config, tall_lambda=0.4, tasks=None,
                          reference_state_dict: Optional[Dict[str, torch.Tensor]] = None, remove_keys=None,
                          device: str = "cuda", return_stats: bool = False):
    """The TALL masks of ``consensus_merge_parameters`` alone -- a launch that writes the packed streams and no merged
    tensor: {task: uint8 tensor}, with ``return_stats`` also the statistics.  The arguments are that function's."""
    _, masks, stats = _tall_run("tall_masks_from_store", compressed_all, bases, original_shapes, tall_lambda, None, 1.0,
                                tasks, None, reference_state_dict, remove_keys, False, True, device)
    return (masks, stats) if return_stats else masks


def _mask_stream_layout(who, names, rows, reference_state_dict, remove_keys):
    """({key: first stream bit}, total bits) of the packed mask streams, TALL's and EMR's: the sorted keys of the
    reference minus ``remove_keys`` (default: ``names``), each at the bit after the one before it.  A parameter of
    ``names`` without a place in them, or with another element count there, raises the named ValueError."""
    skip = set(remove_keys or [])
    if reference_state_dict is None:
        sizes = {n: rows[n] for n in names if n not in skip}
    else:
        sizes = {key: int(x.numel()) for key, x in reference_state_dict.items() if key not in skip}
    for name in names:
        if name not in sizes:
            raise ValueError(f"{who}: parameter {name!r} of the store has no place in the mask streams (it is not a "
                             f"key of reference_state_dict, or remove_keys names it)")
        if sizes[name] != rows[name]:
            raise ValueError(f"{who}: reference_state_dict[{name!r}] has {sizes[name]} elements, the store holds "
                             f"{rows[name]} rows for it")
    bit_base, total_bits = {}, 0
    for key in sorted(sizes):
        bit_base[key] = total_bits
        total_bits += sizes[key]
    return bit_base, total_bits


def _new_mask_streams(T, total_bits, dev):
    """(zeroed int32 streams [T, words], the device table of their T addresses): whole 32-bit words, at least one."""
    streams = torch.zeros((T, max((total_bits + 31) // 32, 1)), dtype=torch.int32, device=dev)
    table = torch.tensor([streams.data_ptr() + 4 * g * streams.shape[1] for g in range(T)], dtype=torch.int64, device=dev)
    return streams, table


def _packed_masks(streams, wanted, total_bits, device):
    """{task: packed uint8 [ceil(total_bits / 8)]} out of the stream tensor, row g for ``wanted[g]``."""
    masks = {}
    for g, t in enumerate(wanted):
        m = streams[g].view(torch.uint8)[:(total_bits + 7) // 8]
        masks[t] = m.cpu() if wants_cpu(device) else m
    return masks


def _popcount_rows(words: torch.Tensor) -> torch.Tensor:
    """Set bits per row of an int32 device tensor [T, W] (int64 [T]); the streams hold 1 / 32 of a model's rows."""
    x = words.to(torch.int64) & 0xffffffff
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0f0f0f0f
    return (((x * 0x01010101) >> 24) & 0xff).sum(dim=1)


def emr_merge_parameters(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict],
                         original_shapes: Dict[str, torch.Size], config, tasks=None,
                         reference_state_dict: Optional[Dict[str, torch.Tensor]] = None, remove_keys=None,
                         device: str = "cuda", return_stats: bool = False):
    """The EMR merge (Huang et al. 2024) of what a store reconstructs, in one pass over the basis, without a task model
    ever being written (the contract is at svdq_plan_emr_elect in include/svdq.h).  With v_t what
    ``reconstruct_task_vectors`` returns for task t and the tasks in sorted-name order: S = the fp32 sum of the values task
    by task, gamma its sign; ``tau_uni = copysign(max |v_t| over the tasks whose sign is gamma, gamma)`` (+0 where S == 0);
    task t's mask is ``v_t * gamma > 0``; its rescaler is ``sum |v_t| / sum (mask_t ? |tau_uni| : 0)`` over all rows, the
    sums in fp64 (1.0 where the second sum is 0).  Task t's model is then ``base + rescaler_t * (mask_t ? tau_uni : 0)``
    (``emr_task_state_dict``).  A task that lacks a parameter contributes nothing on its rows, and its mask is 0 there.
    Nothing is tuned.

    ``tasks``: the names to merge (None = all).  Takes dictionaries backed by a fused run or by ``adopt_artifacts`` and
    refuses what ``dare_merge_parameters`` refuses, under its own name.  The masks are bit-packed as ``numpy.packbits``
    packs them, over the sorted keys of ``reference_state_dict`` minus ``remove_keys`` (default: the store's own
    parameters) -- the layout of a TALL_mask_{T}task file.  Keys of the reference that the store lacks occupy zero bits; a
    store parameter without a place in the reference, or with another element count there, raises a ValueError.

    Returns (unified {param: fp32 tensor}, masks {task: packed uint8 tensor}, rescalers {task: float}); with
    ``return_stats`` also {"abs_sum": {task: A}, "masked_sum": {task: B}, "active": {task: set bits}, "rows": D}.  The
    same arguments give the same bits on every call, the sums included."""
    who = "emr_merge_parameters"
    _, wanted = _store_tasks(compressed_all, tasks, who)
    T = len(wanted)
    names = sorted(compressed_all.keys())
    jobs, rows, live = _ties_jobs(names, wanted, compressed_all, bases, original_shapes, who,
                                  "the EMR merge")      # refusals before device work
    bit_base, total_bits = _mask_stream_layout(who, names, rows, reference_state_dict, remove_keys)
    dev = resolve_device(device)
    D = sum(rows.values())
    unified = {}
    A, B = [0.0] * T, [0.0] * T
    active = [0] * T
    with torch.cuda.device(dev):
        streams, mask_tab = _new_mask_streams(T, total_bits, dev)
        if D > 0:
            state = torch.zeros(int(nat.lib().svdq_emr_state_bytes(T)) // 8, dtype=torch.float64, device=dev)
            for batch, entries in jobs.values():
                plan = batch.plan
                slot_task, task_map, bits = _slot_tables(plan.P, entries, live, bit_base)
                uni_tab, _, rows_dev, _ = _plan_outputs(plan, entries, rows, original_shapes, None, unified, {})
                plan.emr_elect(torch.from_numpy(slot_task).to(plan.device), torch.from_numpy(task_map).to(plan.device), T,
                               torch.from_numpy(bits).to(plan.device), uni_tab, mask_tab, state, rows_dev=rows_dev)
            host = state.cpu().numpy()
            A, B = [float(x) for x in host[:T]], [float(x) for x in host[T:2 * T]]
            if return_stats:
                active = [int(x) for x in _popcount_rows(streams).cpu().tolist()]
        for name in names:
            if name not in unified:      # a store without rows: no launch
                unified[name] = torch.zeros(rows[name], dtype=torch.float32, device=dev)
            unified[name] = _finish_output(unified[name], original_shapes[name], name, {}, device)
        masks = _packed_masks(streams, wanted, total_bits, device)
    rescalers = {t: (A[g] / B[g] if B[g] != 0.0 else 1.0) for g, t in enumerate(wanted)}
    if not return_stats:
        return unified, masks, rescalers
    stats = {"abs_sum": dict(zip(wanted, A)), "masked_sum": dict(zip(wanted, B)), "active": dict(zip(wanted, active)),
             "rows": D}
    return unified, masks, rescalers, stats


def emr_task_state_dict(unified: Dict[str, torch.Tensor], masks: Dict[str, torch.Tensor], rescalers: Dict[str, float],
                        task: str, base_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                        reference_state_dict: Optional[Dict[str, torch.Tensor]] = None, remove_keys=None, rescale=None,
                        device: str = "cuda") -> Dict[str, torch.Tensor]:
    """Task ``task``'s model from what ``emr_merge_parameters`` returned, in ONE launch over the whole model
    (svdq_emr_apply): ``out = base + lambda * (mask ? tau_uni : +0)`` per parameter of ``unified``, the product and the
    sum rounded in fp32, ``lambda = float32(rescalers[task])`` or ``float32(rescale)`` when that is given.  Without
    ``base_state_dict`` (or for a parameter it lacks) the product alone: the task vector EMR serves.  A base that is a
    contiguous fp32 tensor of the parameter's size is added inside the launch; any other base is added afterwards in its
    own arithmetic (``base.to(device) + product``), as ``consensus_merge_parameters`` does.  ``reference_state_dict`` /
    ``remove_keys``: the layout of the mask streams, the ones ``emr_merge_parameters`` was given.  Outputs are fp32, in
    the shapes of ``unified``; keys of the base that ``unified`` lacks are not returned."""
    import math
    import numpy as np
    who = "emr_task_state_dict"
    if task not in masks:
        raise ValueError(f"{who}: unknown task {task!r}: the masks hold {sorted(masks)}")
    lam = rescale if rescale is not None else rescalers.get(task)
    if lam is None:
        raise ValueError(f"{who}: the rescaler of task {task!r} is missing")
    if not _is_number(lam):
        raise ValueError(f"{who}: the rescaler of task {task!r} must be a finite number, got {lam!r}")
    lam32, ok = _as_fp32(lam)
    if not ok:
        raise ValueError(f"{who}: the rescaler of task {task!r} is not finite in fp32: {lam!r}")
    lam32 = float(lam32)
    names = sorted(unified.keys())
    rows = {n: int(unified[n].numel()) for n in names}
    bit_base, total_bits = _mask_stream_layout(who, names, rows, reference_state_dict, remove_keys)
    n_bytes, n_words = (total_bits + 7) // 8, (total_bits + 31) // 32
    stream = masks[task]
    if not (isinstance(stream, torch.Tensor) and stream.dtype is torch.uint8 and stream.dim() == 1
            and stream.numel() == n_bytes):
        raise ValueError(f"{who}: the mask of task {task!r} must be a uint8 tensor of {n_bytes} bytes "
                         f"({total_bits} bits), got {tuple(stream.shape) if isinstance(stream, torch.Tensor) else stream!r}")
    if len(names) > 7679:
        raise ValueError(f"{who}: at most 7679 parameters per call, got {len(names)}")
    dev = resolve_device(device)
    out, later, keep = {}, {}, []
    if not names:
        return out
    with torch.cuda.device(dev):
        # the kernel reads whole 32-bit words: the stream goes into a buffer that has them
        words = torch.zeros(4 * max(n_words, 1), dtype=torch.uint8, device=dev)
        words[:n_bytes] = stream.to(dev)
        P = len(names)
        rows_tab = np.zeros(P, dtype=np.int64)
        bits = np.zeros(P, dtype=np.int64)
        uni_tab = np.zeros(P, dtype=np.int64)
        base_tab = np.zeros(P, dtype=np.int64)
        out_tab = np.zeros(P, dtype=np.int64)
        for i, name in enumerate(names):
            rows_tab[i], bits[i] = rows[name], bit_base[name]
            if rows[name] <= 0:
                out[name] = torch.zeros(unified[name].shape, dtype=torch.float32, device=dev)
                continue
            keep.append(prepare_vector(unified[name], dev))
            uni_tab[i] = keep[-1].data_ptr()
            res = out[name] = torch.empty(rows[name], dtype=torch.float32, device=dev)
            out_tab[i] = res.data_ptr()
            base_tab[i] = _stage_base(name, rows[name], base_state_dict, dev, keep, later)
        tabs =[torch.from_numpy(x).to(dev) for x in (rows_tab, bits, uni_tab, out_tab)]
        base_dev = torch.from_numpy(base_tab).to(dev) if base_tab.any() else None
        if out_tab.any():
            nat.check(nat.lib().svdq_emr_apply(P, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), _ptr(words), lam32,
                                               _ptr(base_dev), _ptr(tabs[3]), _stream_ptr()), "svdq_emr_apply")
        for name in names:
            out[name] = _finish_output(out[name], unified[name].shape, name, later, device)
    return out
