"""Bisecting KMeans trainer (Spark ``BisectingKMeans``, following mllib's algorithm: the tree nodes
are numbered root 1, children ``2 i`` and ``2 i + 1``; a level splits the divisible clusters the last
level made, the largest first when more are divisible than leaves are still allowed).

A bisecting step is a Lloyd step in which a row competes only among the two children of its own
cluster: ``ops.sparse.km_group_step`` with ``W = 2`` (``csrc/clu_kernels.hip`` / ``clu_cpu.cpp``), ``group[r]``
the pair index of the row's leaf or -1, then ``km_centers``. At most 32 clusters split in a level, so a
level is always one pass of 64 centers. Every row term is rounded once to an integer and the
per-cluster sums are exact int64 sums, so host fits, device fits and every world size give the same
tree bit for bit. Under data parallelism (an ambient process group, as for KMeans) each rank holds a
row shard and every iteration all-reduces the int64 block once.

The children of a node start at ``c -+ (1e-4 |c|) u`` with ``u_f = hash_uniform(seed, node index, f)``,
computed on the host from the center copied over. Spark's rules are kept; its own iterates are not
reproduced, because its random numbers are not ours.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ml.linalg import VectorColumn
from ..ops.sparse import KmGroupBlock, _csr, _raise_bad_input, clu_limits, km_centers, km_group_step, km_padded, sim_norms
from ..parallel import dist as D
from ._linear_common import coerce_rows, reduce_statistics
from .kmeans import MEASURES, _Centers, _Problem
from .rf_sampling import hash_uniform

LEVEL_LIMIT = 62                           # levels of a tree whose node indices fit an int64
EPSILON = 2.22e-16                         # a cluster whose cost is at most this per row is not divisible
MAX_SPLITS = 32                            # clusters that split in one level: one pass of 64 centers
ROOT = 1


def _reduced(blk: KmGroupBlock) -> KmGroupBlock:
    if not D.is_dist():
        return blk
    return KmGroupBlock(D.all_reduce_sum(blk.block), blk.F, blk.K, blk.sums, blk.assign, blk.dist)


def _unit(x: np.ndarray, measure: str) -> tuple:
    """A center (cosine: divided by its norm) and its squared norm, as ``kmeans._center_of`` has them."""
    if measure == "cosine":
        nrm = math.sqrt(math.fsum(x * x))
        x = x / nrm if nrm > 0 else x
    return x, math.fsum(x * x)


def children_of(center: np.ndarray, index: int, seed: int, measure: str) -> tuple:
    """``((left, |left|^2), (right, |right|^2))``: ``center -+ (1e-4 |center|) u``, ``u_f =
    hash_uniform(seed, index, f)``; cosine: each child divided by its norm."""
    u = hash_uniform(int(seed), int(index), torch.arange(center.shape[0], dtype=torch.int64)).numpy()
    noise = (1e-4 * math.sqrt(math.fsum(center * center))) * u
    return _unit(center - noise, measure), _unit(center + noise, measure)


def min_divisible_size(m: float, n_global: int) -> int:
    m = float(m)
    return int(math.ceil(m)) if m >= 1.0 else int(math.ceil(m * n_global))


def leaf_order(index, left) -> list:
    """Positions of the leaves, left to right (``left[p]`` the position of the left child, the right
    child follows it, -1 for a leaf)."""
    out, stack = [], [list(index).index(ROOT)]
    while stack:
        p = stack.pop()
        if left[p] < 0:
            out.append(p)
        else:
            stack += [left[p] + 1, left[p]]
    return out


def fit_bisecting_kmeans(features, k: int = 4, weights=None, max_iter: int = 20, seed: int = 566573821,
                         min_divisible_cluster_size: float = 1.0, distance_measure: str = "euclidean", device=None,
                         hot=None, threads: int = 0) -> dict:
    """Fit on a ``VectorColumn`` (rows of this rank under data parallelism). Returns the node arrays
    ``index`` [m] int64, ``cnt`` [m], ``Wq`` [m], ``costq`` [m] (exact), ``cost`` [m], ``center`` [m, F], ``left``
    [m] (the position of the left child, the right one follows it; -1 for a leaf), ``leaves`` (their
    positions, left to right), ``k`` = their number (``<= k`` when nothing more is divisible), ``F``,
    ``cost`` of the leaves summed as ``training_cost``, ``sizes``, ``level_passes`` (the ``km_group_step``
    passes of every level) and the scale exponents."""
    lim = clu_limits()
    k = int(k)
    if not 2 <= k <= lim["max_k"]:
        raise ValueError(f"BisectingKMeans supports k in 2 .. {lim['max_k']}, got {k}")
    if distance_measure not in MEASURES:
        raise ValueError(f"unknown BisectingKMeans distanceMeasure {distance_measure!r} (euclidean, cosine)")
    if int(max_iter) < 0 or not float(min_divisible_cluster_size) > 0.0:
        raise ValueError("BisectingKMeans needs maxIter >= 0 and minDivisibleClusterSize > 0")
    vc0 = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    dev, vc, _, w, n = coerce_rows(vc0, torch.zeros(len(vc0), dtype=torch.float64), weights, device)
    indptr, idx, val = _csr(vc)
    vc = VectorColumn(vc.size, indptr, idx, val)
    F = int(vc.size)
    zero, one = torch.zeros((), dtype=torch.float64, device=dev), torch.ones((), dtype=torch.float64, device=dev)
    (wmax, vmax, nmax), n_global = reduce_statistics(
        [w.max() if w is not None and n else one, val.abs().max().to(torch.float64) if val.numel() else zero,
         sim_norms(indptr, val).max() if n else zero], n, dev)
    if not math.isfinite(wmax) or wmax <= 0:
        raise ValueError("BisectingKMeans weights must be finite and > 0")
    if not math.isfinite(vmax) or not math.isfinite(nmax * nmax):
        raise ValueError("BisectingKMeans requires finite feature values")
    prob = _Problem(vc, w, distance_measure, wmax, vmax, nmax * nmax, n_global, hot=hot, threads=threads)

    # bad input raises on every rank, before anything is drawn
    probe = _Centers(F, 2, distance_measure, dev)
    flag = torch.tensor([prob.step(probe, 2, sums=False, want_rows=False).flag if n else 0], dtype=torch.int64, device=dev)
    if int(D.all_reduce_max(flag)[0] if D.is_dist() else flag[0]):
        _raise_bad_input("km", idx, val, None, w, F)
        raise ValueError("BisectingKMeans: bad input on another rank")
    if n_global < 1:
        raise ValueError("BisectingKMeans needs at least one row")

    def step(group, W: int, G: int, CT, cn, sums: bool, want_rows: bool = False) -> KmGroupBlock:
        return _reduced(km_group_step(vc, group, W, G, CT, cn, distance_measure, prob.k, prob.kw, prob.kc, weights=w,
                                      hot=prob.tables(max(2, W * G)) if sums else None, sums=sums, want_rows=want_rows,
                                      threads=threads, check=False))

    # root: the mean of all rows (cosine: normalised), then its size and cost
    everyone = torch.zeros(n, dtype=torch.int32, device=dev)
    CT0, cn0 = torch.zeros((F, km_padded(2)), dtype=torch.float64, device=dev), \
        torch.zeros(km_padded(2), dtype=torch.float64, device=dev)
    blk = step(everyone, 1, 1, CT0, cn0, sums=True)
    CT, cn, _ = km_centers(blk.S, blk.Wq, CT0, 2, prob.k, prob.kw, distance_measure, threads=threads)
    blk = step(everyone, 1, 1, CT, cn, sums=False)
    index, left = [ROOT], [-1]
    center = [CT[:, 0].cpu().numpy().copy()]
    cnt, Wq, costq = [int(blk.cnt[0])], [int(blk.Wq[0])], [int(blk.costq[0])]
    node_of_row = torch.zeros(n, dtype=torch.int64, device=dev)        # position of every row's leaf

    min_size = min_divisible_size(min_divisible_cluster_size, n_global)
    active, needed, level, level_passes = [0], k - 1, 0, []
    while active and needed > 0 and level < LEVEL_LIMIT:
        divisible = [p for p in active
                     if cnt[p] >= min_size and math.ldexp(float(costq[p]), -prob.kc) > EPSILON * cnt[p]]
        # the largest split, ties to the smaller node index; the pairs are numbered by node index
        chosen = sorted(sorted(divisible, key=lambda p: (-cnt[p], index[p]))[:min(needed, MAX_SPLITS)],
                        key=lambda p: index[p])
        if not chosen:
            break
        G = len(chosen)
        K = max(2, 2 * G)
        Kp = km_padded(K)
        CT_h, cn_h = np.zeros((F, Kp)), np.zeros(Kp)
        for j, p in enumerate(chosen):
            (l, ln), (r, rn) = children_of(center[p], index[p], seed, distance_measure)
            CT_h[:, 2 * j], CT_h[:, 2 * j + 1], cn_h[2 * j], cn_h[2 * j + 1] = l, r, ln, rn
        CT, cn = torch.from_numpy(CT_h).to(dev), torch.from_numpy(cn_h).to(dev)
        pair_of = torch.full((len(index),), -1, dtype=torch.int32, device=dev)
        pair_of[torch.tensor(chosen, dtype=torch.int64, device=dev)] = torch.arange(G, dtype=torch.int32, device=dev)
        group = pair_of[node_of_row]                   # integer gathers only
        passes = 0
        for _ in range(int(max_iter)):
            blk = step(group, 2, G, CT, cn, sums=True)
            CT, cn, moved2 = km_centers(blk.S, blk.Wq, CT, K, prob.k, prob.kw, distance_measure, threads=threads)
            passes += 1
            if float(moved2.max()) == 0.0:             # the rest would repeat
                break
        blk = step(group, 2, G, CT, cn, sums=False, want_rows=True)
        level_passes.append(passes + 1)
        c_cnt, c_wq, c_cost = (t.cpu().numpy() for t in (blk.cnt, blk.Wq, blk.costq))
        CT_h = CT[:, :2 * G].t().contiguous().cpu().numpy()
        leaf_of = torch.zeros(K, dtype=torch.int64, device=dev)       # position of the node a row of child c goes to
        active = []
        for j, p in enumerate(chosen):
            if c_cnt[2 * j] == 0 or c_cnt[2 * j + 1] == 0:            # an empty child undoes the split
                leaf_of[2 * j:2 * j + 2] = p
                continue
            left[p] = len(index)
            for c in (2 * j, 2 * j + 1):
                leaf_of[c] = len(index)
                active.append(len(index))
                index.append(2 * index[p] + (c & 1))
                left.append(-1)
                center.append(CT_h[c].copy())
                cnt.append(int(c_cnt[c]))
                Wq.append(int(c_wq[c]))
                costq.append(int(c_cost[c]))
            needed -= 1
        node_of_row = torch.where(group >= 0, leaf_of[blk.assign.clamp(min=0).to(torch.int64)], node_of_row)
        level += 1

    leaves = leaf_order(index, left)
    cost = [math.ldexp(float(q), -prob.kc) for q in costq]
    return {"index": np.array(index, dtype=np.int64), "cnt": np.array(cnt, dtype=np.int64),
            "Wq": np.array(Wq, dtype=np.int64), "costq": np.array(costq, dtype=np.int64), "cost": np.array(cost),
            "center": np.stack(center), "left": np.array(left, dtype=np.int64), "leaves": leaves, "k": len(leaves),
            "F": F, "training_cost": math.fsum(cost[p] for p in leaves), "sizes": [cnt[p] for p in leaves],
            "level_passes": level_passes, "ek": prob.k, "ekw": prob.kw, "ekc": prob.kc, "measure": distance_measure}


def predict_bisecting(features, index, center, left, distance_measure: str = "euclidean", device=None,
                      threads: int = 0) -> torch.Tensor:
    """The leaf (numbered left to right) of every row, int32 on the column's device. A row descends
    the tree, as in Spark: one assign-only ``km_group_step`` (``W = 2``) per depth over the internal
    nodes of that depth (at most 32 a pass), rows already at a leaf have ``group = -1``; ties go to the
    left child. Raises ``ValueError`` for bad input."""
    vc = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    if device is not None:
        vc = vc.to(torch.device(device))
    index, left = [int(i) for i in index], [int(p) for p in left]
    center = np.asarray(center, dtype=np.float64)
    m, F = center.shape
    if vc.size != F:
        raise ValueError(f"features have size {vc.size}, the model expects {F}")
    dev, n = vc.device, len(vc)
    node_of_row = torch.full((n,), index.index(ROOT), dtype=torch.int64, device=dev)
    internal = sorted((p for p in range(m) if left[p] >= 0), key=lambda p: index[p])
    depths = sorted({index[p].bit_length() for p in internal})
    for depth in depths:
        nodes = [p for p in internal if index[p].bit_length() == depth]
        for lo in range(0, len(nodes), MAX_SPLITS):
            part = nodes[lo:lo + MAX_SPLITS]
            G = len(part)
            K = max(2, 2 * G)
            Kp = km_padded(K)
            CT_h, cn_h = np.zeros((F, Kp)), np.zeros(Kp)
            leaf_of = torch.zeros(K, dtype=torch.int64, device=dev)
            for j, p in enumerate(part):
                for c in (0, 1):
                    CT_h[:, 2 * j + c] = center[left[p] + c]
                    cn_h[2 * j + c] = math.fsum(center[left[p] + c] ** 2)
                    leaf_of[2 * j + c] = left[p] + c
            pair_of = torch.full((m,), -1, dtype=torch.int32, device=dev)
            pair_of[torch.tensor(part, dtype=torch.int64, device=dev)] = torch.arange(G, dtype=torch.int32, device=dev)
            group = pair_of[node_of_row]
            blk = km_group_step(vc, group, 2, G, torch.from_numpy(CT_h).to(dev), torch.from_numpy(cn_h).to(dev),
                                distance_measure, 0, 0, 0, sums=False, want_rows=True, threads=threads)
            node_of_row = torch.where(group >= 0, leaf_of[blk.assign.clamp(min=0).to(torch.int64)], node_of_row)
    number = torch.zeros(m, dtype=torch.int32, device=dev)
    leaves = leaf_order(index, left)
    number[torch.tensor(leaves, dtype=torch.int64, device=dev)] = torch.arange(len(leaves), dtype=torch.int32, device=dev)
    return number[node_of_row]
