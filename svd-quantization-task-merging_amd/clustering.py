"""
Task clustering for cluster-weighted merging (reference
src/svd_hybrid/clustering.py:55-425).

The reference flattens every task vector into one row of a host ``[N, sum D]`` numpy matrix
(clustering.py:55-120; 24 GB at ViT-L-14 x 20) and hands it to scikit-learn.  K-means and Ward linkage
only ever look at distances between the N rows and their means, i.e. at the N x N Gram matrix of the
rows.  Here the Gram comes from one streaming pass over the task deltas where they already live
(``svdq_task_gram``: fp32 MFMA per 256-row block, fp64 across blocks, deterministic), is all-reduced
across ranks when the parameters are sharded (N*N doubles), and an exact N-dimensional embedding
``E`` with ``E E^T = Gram`` replaces the feature matrix.  scikit-learn / scipy then run on N x N
numbers with the reference's arguments (KMeans(n_clusters=k, random_state=42, n_init=10); ward).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .pipeline import CompressPlan, native_input_dtype, prepare_input, resolve_device


def scatter_task_gram(total: np.ndarray, gram: np.ndarray, present: List[str], tasks: List[str]) -> None:
    """Add one plan's Gram (rows / columns = the tasks in ``present``, the plan's task order) into the run's N x N
    matrix ``total`` (rows / columns = ``tasks``).  A task the plan's parameters lack counts as zeros for them
    (flatten_task_vectors), i.e. its rows and columns get nothing."""
    pos = {t: i for i, t in enumerate(tasks)}
    idx = np.array([pos[t] for t in present], dtype=np.int64)
    total[np.ix_(idx, idx)] += np.asarray(gram, dtype=np.float64).reshape(len(present), len(present))


def recorded_task_gram(bases, tasks: List[str]):
    """The task Gram that the plans behind ``bases`` (driver.build_bases with the by-product enabled) recorded as they
    ran: (G [N, N] fp64 in the order of ``tasks``, the set of parameter names it covers), or None when nothing was
    recorded or a recorded task is not in ``tasks``."""
    seen, records = set(), []
    for b in (bases or {}).values():
        art = b.get("masked") if isinstance(b, dict) else None
        batch = getattr(art, "_batch", None)
        rec = getattr(batch[0], "task_gram", None) if batch is not None else None
        if rec is not None and id(batch[0]) not in seen:
            seen.add(id(batch[0]))
            records.append(rec)
    if not records or any(t not in tasks for r in records for t in r["tasks"]):
        return None
    G = np.zeros((len(tasks), len(tasks)), dtype=np.float64)
    covered = set()
    for r in records:
        gram = r["gram"]
        scatter_task_gram(G, gram.cpu().numpy() if isinstance(gram, torch.Tensor) else gram, r["tasks"], tasks)
        covered.update(r["names"])
    return G, covered


def task_gram(task_vectors: Dict[str, Dict[str, torch.Tensor]], device="cuda", *, process_group=None,
              bases=None) -> Tuple[np.ndarray, List[str]]:
    """N x N inner products (fp64, host) of the flattened task vectors, tasks in sorted order.

    ``bases`` (from driver.build_bases / run_basis_and_compress[_from_checkpoints] with the task-Gram by-product, the
    default of a cluster-weighted config): the Gram its plans recorded while compressing is taken as it is, and only the
    parameters it does not cover (the masked ones, here in full, unmasked form) are read -- in the common case none,
    and then ``task_vectors`` only has to name the tasks.

    Same row/column conventions as flatten_task_vectors (clustering.py:55-120): tasks sorted by name,
    parameters the union over tasks, a parameter a task lacks counts as zeros.  With ``process_group``
    (or an initialised default group and ``process_group=True``) each rank passes only the parameters it
    owns and the Gram is summed over ranks -- the one N*N all-reduce of SURVEY 8(e)."""
    dev = resolve_device(device)
    tasks = sorted(task_vectors.keys())
    names = sorted({n for tv in task_vectors.values() for n in tv.keys()})
    N = len(tasks)
    vectors, rows = [], []
    recorded = recorded_task_gram(bases, tasks) if bases is not None else None
    if recorded is not None:
        names = [n for n in names if n not in recorded[1]]
    # one plan for the whole model: all fp16 / all bf16 task tensors are read as they are, any mix as fp32 copies
    idt = native_input_dtype(tv[n] for tv in task_vectors.values() for n in tv.keys())
    with torch.cuda.device(dev):
        for name in names:
            ref = next(tv[name] for tv in task_vectors.values() if name in tv)
            if ref.numel() == 0:
                continue
            vs = []
            for t in tasks:
                if name in task_vectors[t]:
                    vs.append(prepare_input(task_vectors[t][name], dev, idt))
                else:
                    vs.append(torch.zeros(ref.numel(), dtype=idt, device=dev))
            vectors.append(vs)
            rows.append(ref.numel())
        if vectors:
            plan = CompressPlan(rows, N, center=False, device=dev, gram_only=True, input_dtype=idt)
            G = plan.task_gram(plan.pointer_table(vectors))
        else:
            G = torch.zeros((N, N), dtype=torch.float64, device=dev)
        if recorded is not None:
            G = G + torch.from_numpy(recorded[0]).to(dev)
        if process_group is not None:
            from .shard import all_reduce_gram
            all_reduce_gram(G, None if process_group is True else process_group)
        out = G.cpu().numpy()
        if vectors:
            plan.close()
    return out, tasks


def assemble_task_gram(per_param: Dict[str, List[Tuple[np.ndarray, List[str]]]], tasks: List[str]) -> np.ndarray:
    """The store's N x N Gram (rows / columns = ``tasks``) from per-parameter pieces {parameter: [(matrix, the tasks
    its rows / columns stand for)]}: every matrix is added at its tasks' positions (``scatter_task_gram``), parameters in
    sorted-name order, so the sum has one association whatever route produced the pieces.  A task that lacks a parameter
    gets nothing from it (flatten_task_vectors' zeros).  A non-finite entry in a parameter's matrix is a ``ValueError``
    that names the parameter: one NaN would otherwise spread over every label."""
    G = np.zeros((len(tasks), len(tasks)), dtype=np.float64)
    for name in sorted(per_param.keys()):
        for gram, present in per_param[name]:
            gram = np.asarray(gram, dtype=np.float64).reshape(len(present), len(present))
            if not np.isfinite(gram).all():
                raise ValueError(f"the task Gram of parameter {name!r} is not finite: its stored artifacts hold a NaN or "
                                 f"Inf (basis, mean or coefficients)")
            scatter_task_gram(G, gram, present, tasks)
    return G


def _artifact_tasks(per_task) -> List[str]:
    meta = getattr(per_task, "_meta", None)      # a plan-backed entry names its tasks without being materialised
    return list(meta["have"]) if meta else list(per_task.keys())


def task_gram_from_artifacts(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict], device="cuda",
                             basis_report: bool = False):
    """``task_gram`` of a STORE: (G [N, N] fp64 on the host, the task names in sorted order) of the task vectors the
    stored artifacts reconstruct, ``delta_t = U c_t + mean`` per parameter and region -- what the reference's cluster
    weighting (flatten_task_vectors clustering.py:55-120, cluster_tasks :198-245) would see after
    ``reconstruct_task_vectors`` for every task, without a checkpoint and without writing one reconstructed model.
    Conventions as ``task_gram``: tasks sorted by name, parameters the union over tasks, a parameter a task lacks counts
    as zeros.  No weight, no scale: ``svd_noise_shrink`` is NOT applied (the reference clusters raw task vectors).

    Entries that ``merge._batched_entry`` accepts -- a fused run's dictionaries, ``adopt_artifacts``' output -- take ONE
    ``svdq_plan_store_gram`` per distinct plan (``CompressPlan.store_gram``: a pass over the basis and the mean, 2 r + 4
    bytes per row with an fp16 basis).  Signal and noise entries of a masked run both contribute: their rows are disjoint,
    so the sum is the Gram of the full reconstructed vectors WHEN the run stored noise regions (svd_include_noise), and of
    their signal part alone when it did not -- the store then holds nothing of the other rows.  Any other entry goes per
    (parameter, region, task) through ``merge_parameter`` on that task alone with weight 1.0, and the matrix is formed
    with torch in fp64.  The per-parameter matrices are added by task name in sorted parameter order
    (``assemble_task_gram``); a non-finite one is a ``ValueError`` naming the parameter.

    ``basis_report=True``: returns ``(G, tasks, report)`` with report = {"param [region]": max |U^T U - I|}, the
    orthonormality of every stored (rounded, extended, caller-made) basis -- from the same pass."""
    from .merge import _batched_entry, merge_parameter
    from .rtvq import RTVQQuantizer
    dev = resolve_device(device)
    names = sorted(compressed_all.keys())
    tasks = sorted({t for n in names for t in _artifact_tasks(compressed_all[n])})
    jobs, rest = {}, []      # id(plan) -> (plan batch, {entry index: (name, region, meta)})
    for name in names:
        got = _batched_entry(name, compressed_all, bases)
        if got is None:
            rest.append(name)
            continue
        batch, i, meta = got
        jobs.setdefault(id(batch.plan), (batch, {}))[1][i] = (name, "masked", meta)
        if meta["noise"] is not None:
            nb, j = meta["noise"]
            jobs.setdefault(id(nb.plan), (nb, {}))[1][j] = (name, "noise", meta)
    per_param: Dict[str, list] = {}
    report: Dict[str, float] = {}
    with torch.cuda.device(dev):
        for batch, entries in jobs.values():
            plan = batch.plan
            out = plan.store_gram(basis_gram=basis_report)
            G = (out[0] if basis_report else out).cpu().numpy()      # the one device-to-host copy of the plan
            B = out[1].cpu().numpy() if basis_report else None
            for i, (name, region, meta) in entries.items():
                if int(batch.small.rows[i]) <= 0:
                    continue
                tasks_i = batch.task_names[i]
                sel = [q for q, t in enumerate(tasks_i) if t in meta["have"]]
                per_param.setdefault(name, []).append((G[i][np.ix_(sel, sel)], [tasks_i[q] for q in sel]))
                if basis_report:
                    r = int(batch.small.r[i])
                    report[f"{name} [{region}]"] = float(np.abs(B[i][:r, :r] - np.eye(r)).max()) if r else 0.0
        quantizer = RTVQQuantizer()      # only dequantizes: the payloads carry their own widths
        for name in rest:
            per_task, b = compressed_all[name], bases.get(name) or {}
            for region, key in (("masked", "masked"), ("noise", "unmasked")):
                rb = b.get(region)
                if rb is None:
                    continue
                present = sorted(t for t, a in per_task.items() if isinstance(a, dict) and a.get(key) is not None)
                if not present:
                    continue
                rows = int(rb["U_high"].shape[0] if rb["U_high"].dim() == 2 else rb["U_low"].shape[0])
                # merge_parameter on one task with weight 1.0 is that task's own reconstruction; the region rides in the
                # "masked" slot so that neither a mask nor noise_shrink comes into it
                X = torch.stack([merge_parameter(name, {t: {"masked": per_task[t][key]}}, {"masked": rb}, {t: 1.0},
                                                 quantizer, torch.Size([rows]), device=dev).double()
                                 for t in present])
                per_param.setdefault(name, []).append(((X @ X.T).cpu().numpy(), present))
                if basis_report:
                    U = torch.cat([u.to(dev).double() for u in (rb["U_high"], rb["U_low"]) if u.dim() == 2 and u.shape[1]],
                                  dim=1) if rows else torch.zeros((0, 0), dtype=torch.float64, device=dev)
                    r = int(U.shape[1])
                    report[f"{name} [{region}]"] = float((U.T @ U - torch.eye(r, dtype=torch.float64, device=dev))
                                                         .abs().max()) if r else 0.0
    G = assemble_task_gram(per_param, tasks)
    return (G, tasks, report) if basis_report else (G, tasks)


def cluster_tasks_from_artifacts(compressed_all: Dict[str, Dict[str, Dict]], bases: Dict[str, Dict], k: int,
                                 method: str = "kmeans", device="cuda") -> Dict[str, int]:
    """``cluster_tasks`` (clustering.py:198-245) for a store: the labels of the task vectors the stored artifacts
    reconstruct, from ``task_gram_from_artifacts``."""
    if method not in ("kmeans", "hierarchical"):
        raise ValueError(f"Unknown clustering method: {method}")
    G, tasks = task_gram_from_artifacts(compressed_all, bases, device=device)
    return cluster_from_gram(G, tasks, k, method)


def flatten_task_vectors(task_vectors: Dict[str, Dict[str, torch.Tensor]]) -> Tuple[np.ndarray, List[str]]:
    """Reference clustering.py:55-120: the [N, sum D] feature matrix (rows = tasks in sorted-name order, parameters in
    sorted-name order, zeros where a task lacks a parameter) and the task names.  Kept for API compatibility only:
    nothing in this package needs the matrix -- ``cluster_tasks`` works from the N x N Gram (``task_gram``), which is
    all the clustering ever uses of it -- and at ViT-L-14 x 20 it is 24 GB of host memory."""
    names = sorted(task_vectors.keys())
    params = sorted({p for tv in task_vectors.values() for p in tv})
    shape_of = {p: next(tv[p] for tv in task_vectors.values() if p in tv) for p in params}
    rows = []
    for t in names:
        tv = task_vectors[t]
        parts = [(tv[p] if p in tv else torch.zeros_like(shape_of[p])).flatten() for p in params]
        rows.append(torch.cat(parts, dim=0).cpu().numpy())
    return np.stack(rows, axis=0), names


def gram_embedding(G: np.ndarray) -> np.ndarray:
    """Rows e_i in R^N with e_i . e_j = G_ij (eigen-decomposition, negative round-off clipped)."""
    lam, Q = np.linalg.eigh((G + G.T) * 0.5)
    return Q * np.sqrt(np.clip(lam, 0.0, None))[None, :]


def normalized_gram(G: np.ndarray) -> np.ndarray:
    """Gram of ``features / (||features|| + 1e-8)`` (clustering.py:230-231)."""
    norm = np.sqrt(np.clip(np.diag(G), 0.0, None)) + 1e-8
    return G / norm[:, None] / norm[None, :]


def compute_kmeans_clustering(features: np.ndarray, k: int, random_state: int = 42) -> np.ndarray:
    """clustering.py:123-156."""
    from sklearn.cluster import KMeans
    if k <= 0 or k > features.shape[0]:
        raise ValueError(f"Invalid k={k} for {features.shape[0]} samples")
    return KMeans(n_clusters=k, random_state=random_state, n_init=10).fit_predict(features)


def compute_hierarchical_clustering(features: np.ndarray, k: int, method: str = "ward") -> np.ndarray:
    """clustering.py:159-195."""
    from scipy.cluster.hierarchy import fcluster, linkage
    if k <= 0 or k > features.shape[0]:
        raise ValueError(f"Invalid k={k} for {features.shape[0]} samples")
    return fcluster(linkage(features, method=method), k, criterion="maxclust") - 1


def cluster_from_gram(G: np.ndarray, task_names: List[str], k: int, method: str = "kmeans") -> Dict[str, int]:
    feats = gram_embedding(normalized_gram(G))
    if method == "kmeans":
        labels = compute_kmeans_clustering(feats, k)
    elif method == "hierarchical":
        labels = compute_hierarchical_clustering(feats, k)
    else:
        raise ValueError(f"Unknown clustering method: {method}")
    return {name: int(lab) for name, lab in zip(task_names, labels)}


def cluster_tasks(task_vectors: Dict[str, Dict[str, torch.Tensor]], k: int, method: str = "kmeans",
                  device="cuda", process_group=None, bases=None) -> Dict[str, int]:
    """clustering.py:198-245: unit-normalised task vectors -> k-means / Ward labels per task name."""
    if method not in ("kmeans", "hierarchical"):
        raise ValueError(f"Unknown clustering method: {method}")
    G, tasks = task_gram(task_vectors, device, process_group=process_group, bases=bases)
    return cluster_from_gram(G, tasks, k, method)


def get_cluster_members(cluster_assignments: Dict[str, int]) -> Dict[int, List[str]]:
    """clustering.py:248-275."""
    clusters: Dict[int, List[str]] = {}
    for task, cid in cluster_assignments.items():
        clusters.setdefault(cid, []).append(task)
    return clusters


def cluster_statistics_from_gram(G: np.ndarray, task_names: List[str], cluster_assignments: Dict[str, int]
                                 ) -> Dict[int, Dict]:
    """||x_i - centroid||^2 = G_ii - 2 mean_j G_ij + mean_jl G_jl over the members j, l of the cluster."""
    index = {name: i for i, name in enumerate(task_names)}
    stats = {}
    for cid, members in get_cluster_members(cluster_assignments).items():
        idx = np.array([index[m] for m in members])
        sub = G[np.ix_(idx, idx)]
        d2 = np.diag(sub) - 2.0 * sub.mean(axis=1) + sub.mean()
        d = np.sqrt(np.clip(d2, 0.0, None))
        stats[cid] = {"size": len(members), "members": members,
                      "mean_distance_to_centroid": float(d.mean()),
                      "max_distance_to_centroid": float(d.max()),
                      "min_distance_to_centroid": float(d.min())}
    return stats


def compute_cluster_statistics(task_vectors: Dict[str, Dict[str, torch.Tensor]], cluster_assignments: Dict[str, int],
                               device="cuda", process_group=None, bases=None) -> Dict[int, Dict]:
    """clustering.py:278-316 (distances of the UN-normalised task vectors to their cluster centroid)."""
    G, tasks = task_gram(task_vectors, device, process_group=process_group, bases=bases)
    return cluster_statistics_from_gram(G, tasks, cluster_assignments)


def merge_by_cluster(task_vectors: Dict[str, Dict[str, torch.Tensor]], cluster_assignments: Dict[str, int],
                     weights: Dict[str, float], device: str = "cpu") -> Dict[int, Dict[str, torch.Tensor]]:
    """clustering.py:319-371: per cluster, weighted average of the members' task vectors."""
    from .weighting import apply_weights_to_tensors
    merged = {}
    for cid, members in get_cluster_members(cluster_assignments).items():
        w = {m: weights.get(m, 1.0) for m in members}
        total = sum(w.values())
        w = {m: v / total for m, v in w.items()}
        names = {n for m in members for n in task_vectors[m].keys()}
        merged[cid] = {}
        for n in names:
            present = {m: task_vectors[m][n] for m in members if n in task_vectors[m]}
            if present:
                merged[cid][n] = apply_weights_to_tensors(present, w, device)
    return merged


def merge_cluster_results(cluster_merged: Dict[int, Dict[str, torch.Tensor]], cluster_performance: Dict[int, float],
                          device: str = "cpu") -> Dict[str, torch.Tensor]:
    """clustering.py:374-425: softmax(cluster performance) (uniform when empty) average across clusters."""
    from .weighting import apply_weights_to_tensors
    if not cluster_merged:
        return {}
    cids = list(cluster_merged.keys())
    if cluster_performance:
        share = torch.softmax(torch.tensor([cluster_performance.get(c, 1.0) for c in cids]), dim=0)
    else:
        share = torch.ones(len(cids)) / len(cids)
    w = {c: s.item() for c, s in zip(cids, share)}
    names = {n for params in cluster_merged.values() for n in params.keys()}
    out = {}
    for n in names:
        present = {c: cluster_merged[c][n] for c in cids if n in cluster_merged[c]}
        if present:
            out[n] = apply_weights_to_tensors(present, w, device)
    return out
