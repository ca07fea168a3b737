"""Spark's silhouette (``ClusteringEvaluator``) as two exact passes over the CSR.

Spark's closed form needs per-cluster sums only, so the measure is not O(n^2): pass A is
``ops.sparse.km_group_step`` with ``W = 1``, ``group = prediction`` and zero centers, which gives every
cluster's exact int64 coordinate sums ``S``, weight sum ``Wq``, row count and (euclidean: ``d = |x|^2``)
the sum of the weighted squared norms; ``km_centers`` turns ``S`` and ``Wq`` into the means. Pass B is
``ops.sparse.sil_score``: every row's coefficient and the exact sums ``silq`` and ``wq``. Under data
parallelism (an ambient process group, as for KMeans) each rank holds a row shard: the maxima that fix
the scale exponents are all-reduced with MAX, the block of pass A and ``[silq, wq]`` of pass B with one
SUM each. Every sum is an integer, so host, device and every world size give the same bits.

The singleton rule is ``cnt == 1`` (Spark: ``weightSum == weight``): a fixed-point weight sum of one
row need not equal its weight.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ml.linalg import VectorColumn
from ..ops.sparse import (KmGroupBlock, _csr, _raise_bad_input, clu_limits, km_centers, km_group_step, km_padded,
                          nb_scale_exponent, sil_score, sim_norms)
from ..parallel import dist as D
from ._linear_common import coerce_rows, reduce_statistics

MEASURES = {"squaredEuclidean": "euclidean", "euclidean": "euclidean", "cosine": "cosine"}


def _predictions(prediction, n: int, dev) -> torch.Tensor:
    """The predictions as int64 on ``dev``; ``ValueError`` unless there is one integer per row."""
    p = torch.as_tensor(np.asarray(prediction) if not isinstance(prediction, torch.Tensor) else prediction)
    if p.numel() != n:
        raise ValueError("the silhouette needs one prediction per row")
    p = p.to(dev).view(-1)
    if p.dtype.is_floating_point:
        if not bool(torch.all(torch.isfinite(p) & (p == torch.floor(p)))):
            raise ValueError("predictions must be integers")
    return p.to(torch.int64)


def silhouette(features, prediction, weights=None, measure: str = "squaredEuclidean", device=None,
               want_rows: bool = False, hot=None, threads: int = 0) -> dict:
    """The silhouette of a clustering of a ``VectorColumn`` (rows of this rank under data
    parallelism). Returns ``value`` = ``silq 2^-ks / (wq 2^-kw)``, the exact integers ``silq`` and ``wq``,
    ``k`` (the largest prediction over all ranks + 1), the per-cluster ``cnt``, ``Wq`` and ``costq`` of pass
    A, the scale exponents ``ek`` / ``ekw`` / ``ekc`` / ``eks`` and, with ``want_rows``, ``s``: this rank's
    per-row coefficients (fp64, on the column's device). Raises ``ValueError`` for an unknown measure,
    predictions that are no integers >= 0, more than ``max_k`` clusters, fewer than two non-empty
    clusters and KMeans' bad-input cases, on every rank."""
    if measure not in MEASURES:
        raise ValueError(f"unknown silhouette distanceMeasure {measure!r} (squaredEuclidean, cosine)")
    m = MEASURES[measure]
    cos = m == "cosine"
    lim = clu_limits()
    vc0 = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    dev, vc, _, w, n = coerce_rows(vc0, torch.zeros(len(vc0), dtype=torch.float64), weights, device)
    indptr, idx, val = _csr(vc)
    vc = VectorColumn(vc.size, indptr, idx, val)
    F = int(vc.size)
    pred = _predictions(prediction, n, dev)
    zero, one = torch.zeros((), dtype=torch.float64, device=dev), torch.ones((), dtype=torch.float64, device=dev)
    # (largest weight, largest |value|, largest row norm, largest prediction, - smallest prediction)
    (wmax, vmax, nmax, pmax, pmin), n_global = reduce_statistics(
        [w.max() if w is not None and n else one, val.abs().max().to(torch.float64) if val.numel() else zero,
         sim_norms(indptr, val).max() if n else zero, pred.max().to(torch.float64) if n else zero,
         -pred.min().to(torch.float64) if n else zero], n, dev)
    if not math.isfinite(wmax) or wmax <= 0:
        raise ValueError("silhouette weights must be finite and > 0")
    if not math.isfinite(vmax) or not math.isfinite(nmax * nmax):
        raise ValueError("the silhouette requires finite feature values")
    if pmin > 0:
        raise ValueError("predictions must be >= 0")
    G = int(pmax) + 1
    if G > lim["max_k"]:
        raise ValueError(f"the silhouette supports up to {lim['max_k']} clusters, got {G}")
    K, xnmax = max(2, G), nmax * nmax
    k = nb_scale_exponent(wmax if cos else wmax * vmax, n_global)
    kw = nb_scale_exponent(wmax, n_global)
    kc = nb_scale_exponent(wmax if cos else wmax * xnmax, n_global)
    ks = nb_scale_exponent(2.0 * wmax, n_global)
    Kp = km_padded(K)
    group = pred.to(torch.int32)

    # pass A: the per-cluster sums against zero centers (euclidean: d = |x|^2, so costq sums w |x|^2)
    CT0 = torch.zeros((F, Kp), dtype=torch.float64, device=dev)
    blk = km_group_step(vc, group, 1, G, CT0, torch.zeros(Kp, dtype=torch.float64, device=dev), m, k, kw, kc, weights=w,
                        hot=hot, sums=True, threads=threads, check=False)
    block = D.all_reduce_sum(blk.block) if D.is_dist() else blk.block
    if int(block[-1]):
        if blk.flag:
            _raise_bad_input("km", idx, val, None, w, F)
        raise ValueError("silhouette: bad input on another rank")
    blk = KmGroupBlock(block, F, K, True)
    cnt = blk.cnt.cpu().numpy()
    if int((cnt > 0).sum()) < 2:
        raise ValueError("the silhouette needs at least two non-empty clusters")
    MT, _, _ = km_centers(blk.S, blk.Wq, CT0, K, k, kw, "euclidean", threads=threads)
    Wq, costq = blk.Wq.cpu().numpy(), blk.costq.cpu().numpy()
    nw, psi = np.zeros(Kp), np.zeros(Kp)
    nw[:K] = np.ldexp(Wq.astype(np.float64), -kw)
    if not cos:
        live = nw[:K] > 0
        psi[:K][live] = np.ldexp(costq.astype(np.float64), -kc)[live] / nw[:K][live]
    cnt32 = np.zeros(Kp, dtype=np.int32)
    cnt32[:K] = cnt

    # pass B: the coefficients
    args = (vc, group, K, MT, torch.from_numpy(psi).to(dev), torch.from_numpy(nw).to(dev), torch.from_numpy(cnt32).to(dev),
            m, ks, kw)
    sil = sil_score(*args, weights=w, want_rows=want_rows, threads=threads, check=False)
    out = D.all_reduce_sum(sil.block) if D.is_dist() else sil.block
    silq, wq, flag = (int(v) for v in out.cpu())
    if flag:
        if sil.flag:
            sil_score(*args, weights=w, threads=threads)           # names the bad input
        raise ValueError("silhouette: bad input on another rank")
    res = {"value": math.ldexp(float(silq), -ks) / math.ldexp(float(wq), -kw), "silq": silq, "wq": wq, "k": G, "F": F,
           "cnt": cnt[:G].tolist(), "Wq": Wq[:G].tolist(), "costq": costq[:G].tolist(), "ek": k, "ekw": kw, "ekc": kc,
           "eks": ks, "measure": m}
    if want_rows:
        res["s"] = sil.s
    return res
