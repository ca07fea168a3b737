"""KMeans trainer (Spark ``KMeans``: Lloyd iterations, ``random`` and ``k-means||`` seeding, the
euclidean and the cosine measure).

An iteration is one ``ops.sparse.km_step`` pass (``csrc/km_kernels.hip`` / ``km_cpu.cpp``) and one
``km_centers``: every row's distances are summed in a fixed order, every term that leaves a row is
scaled by a power of two and rounded once to an integer, and the per-cluster sums are exact int64
sums. Integer adds commute, so host fits, device fits and every world size give the same centers
bit for bit. Under data parallelism (an ambient process group, as for Naive Bayes) each rank holds
a row shard: the maxima that fix the scale exponents are all-reduced with MAX, then every iteration
all-reduces the int64 block ``[S, Wq, cnt, costq]`` once. The host reads one small tuple an
iteration: ``moved2`` [K] and ``costq``.

Every draw is keyed by ``(seed, stage, global row index)`` through ``rf_sampling.hash_uniform``, and
the sampling arithmetic runs on the host on values copied from the device, so a fit is a pure
function of (data, params). Spark's stopping rules are kept; its own iterates are not reproduced,
because its random numbers are not ours.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ml.linalg import VectorColumn
from ..ops.sparse import (KmBlock, _csr, _raise_bad_input, hot_tables, km_centers, km_limits, km_padded, km_step,
                          nb_scale_exponent, sim_norms)
from ..parallel import dist as D
from ._linear_common import coerce_rows, reduce_statistics
from .rf_sampling import hash_uniform

INIT_MODES = ("random", "k-means||")
MEASURES = ("euclidean", "cosine")
LOCAL_ITERATIONS = 30                      # Lloyd iterations on the candidates (Spark's LocalKMeans)
# stages of the draws: hash_uniform(seed, stage, global row index)
_STAGE_RANDOM, _STAGE_FIRST, _STAGE_LOCAL, _STAGE_ROUND = 1, 2, 3, 16      # round r draws with _STAGE_ROUND + r


class _Rows:
    """A few rows on the host: ``(global row index, feature ids int32, values float64)`` each."""

    def __init__(self, gidx=(), idx=(), val=()):
        self.gidx, self.idx, self.val = list(gidx), list(idx), list(val)

    def __len__(self) -> int:
        return len(self.idx)

    def extend(self, other: "_Rows") -> None:
        self.gidx += other.gidx
        self.idx += other.idx
        self.val += other.val

    def column(self, F: int, dev) -> VectorColumn:
        ptr = np.zeros(len(self) + 1, dtype=np.int64)
        np.cumsum([len(i) for i in self.idx], out=ptr[1:])
        idx = np.concatenate(self.idx) if len(self) else np.zeros(0, np.int32)
        val = np.concatenate(self.val) if len(self) else np.zeros(0, np.float64)
        return VectorColumn(F, torch.from_numpy(ptr).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev),
                            torch.from_numpy(val.astype(np.float64)).to(dev))


def _gather_rows(vc: VectorColumn, local: torch.Tensor, offset: int, dev) -> _Rows:
    """The rows ``local`` (ascending local indices) of every rank's shard, in rank order."""
    sub = vc.take(local.to(vc.device))
    ptr, idx, val = sub.csr()
    lens = (ptr[1:] - ptr[:-1]).to(dev)
    gidx = (local.to(torch.int64) + offset).to(dev)
    idx, val = idx.to(torch.int32).to(dev), val.to(torch.float64).to(dev)
    if D.is_dist():
        lens, gidx = D.all_gather_var(lens, gidx)
        idx, val = D.all_gather_var(idx, val)
    lens, gidx, idx, val = (t.cpu().numpy() for t in (lens, gidx, idx, val))
    ends = np.cumsum(lens)
    return _Rows(gidx.tolist(), [idx[e - n:e] for n, e in zip(lens, ends)], [val[e - n:e] for n, e in zip(lens, ends)])


def _center_of(idx: np.ndarray, val: np.ndarray, measure: str) -> tuple:
    """A row as a center: its values (cosine: divided by the norm) and its squared norm."""
    x = val.astype(np.float64)
    if measure == "cosine":
        x = x / math.sqrt(math.fsum(x * x))
    return x, math.fsum(x * x)


class _Centers:
    """``CT`` [F, Kp] and ``cn`` [Kp] on the device, filled a column at a time from sparse rows."""

    def __init__(self, F: int, K: int, measure: str, dev):
        self.F, self.K, self.measure, self.dev = F, K, measure, dev
        self.CT = torch.zeros((F, km_padded(K)), dtype=torch.float64, device=dev)
        self.cn = torch.zeros(km_padded(K), dtype=torch.float64, device=dev)

    def set(self, c: int, idx: np.ndarray, val: np.ndarray) -> None:
        x, nn = _center_of(idx, val, self.measure)
        self.CT[:, c] = 0.0
        self.CT[torch.from_numpy(idx.astype(np.int64)).to(self.dev), c] = torch.from_numpy(x).to(self.dev)
        self.cn[c] = nn

    def fill(self, idx: np.ndarray, val: np.ndarray) -> None:
        """Every column holds this row: a center that repeats an earlier one wins no tie."""
        x, nn = _center_of(idx, val, self.measure)
        self.CT.zero_()
        self.CT[torch.from_numpy(idx.astype(np.int64)).to(self.dev), :self.K] = torch.from_numpy(x).to(self.dev)[:, None]
        self.cn[:self.K] = nn

    @classmethod
    def of_rows(cls, rows: _Rows, F: int, measure: str, dev) -> "_Centers":
        """The rows as centers; one row is stored twice, a pass takes at least two centers."""
        K = max(len(rows), 2)
        cs = cls(F, K, measure, dev)
        for c in range(K):
            j = min(c, len(rows) - 1)
            cs.set(c, rows.idx[j], rows.val[j])
        return cs


class _Problem:
    """A CSR column with weights, the measure and the scale exponents of its passes."""

    def __init__(self, vc, w, measure: str, wmax: float, vmax: float, xnmax: float, n_global: int, hot=None,
                 threads: int = 0):
        self.vc, self.w, self.measure, self.threads = vc, w, measure, threads
        self.F = int(vc.size)
        self.dev = vc.device
        cos = measure == "cosine"
        self.k = nb_scale_exponent(wmax if cos else wmax * vmax, n_global)
        self.kw = nb_scale_exponent(wmax, n_global)
        self.kc = nb_scale_exponent(2.0 * wmax if cos else 8.0 * wmax * xnmax, n_global)
        self._hot, self._tables = hot, {}

    def tables(self, K: int) -> tuple:
        if K not in self._tables:
            self._tables[K] = hot_tables(*_csr(self.vc), self.F, K, self._hot)
        return self._tables[K]

    def step(self, cs, K: int, sums: bool, want_rows: bool) -> KmBlock:
        CT, cn = (cs.CT, cs.cn) if isinstance(cs, _Centers) else cs
        return km_step(self.vc, CT, cn, K, self.measure, self.k, self.kw, self.kc, weights=self.w,
                       hot=self.tables(K) if sums else None, sums=sums, want_rows=want_rows, threads=self.threads,
                       check=False)

    def nearest(self, rows: _Rows, best=None, base: int = 0) -> tuple:
        """``(dist [n], index [n])`` of every row's nearest of ``rows`` (passes of at most ``max_k``
        centers, combined with an elementwise minimum, ties to the earlier), folded into ``best``;
        the indices count from ``base``."""
        step = int(km_limits()["max_k"])
        for lo in range(0, len(rows), step):
            part = _Rows(rows.gidx[lo:lo + step], rows.idx[lo:lo + step], rows.val[lo:lo + step])
            cs = _Centers.of_rows(part, self.F, self.measure, self.dev)
            blk = self.step(cs, cs.K, sums=False, want_rows=True)
            d, a = blk.dist, blk.assign.to(torch.int64) + (base + lo)
            if best is None:
                best = (d, a)
            else:
                closer = d < best[0]
                best = (torch.where(closer, d, best[0]), torch.where(closer, a, best[1]))
        return best

    def lloyd(self, CT, cn, K: int, max_iter: int, tol: float, until_stable: bool = False) -> tuple:
        """Lloyd iterations from ``(CT, cn)``: ``(CT, cn, iterations)``. Stops when no center moved
        more than ``tol`` (``until_stable``: when no row changed its cluster) or at ``max_iter``."""
        it, prev = 0, None
        while it < max_iter:
            blk = self.step((CT, cn), K, sums=True, want_rows=until_stable)
            block = blk.block
            if D.is_dist() and not until_stable:
                block = D.all_reduce_sum(block)
                blk = KmBlock(block, self.F, K, True)
            if until_stable and prev is not None and torch.equal(prev, blk.assign):
                break
            prev = blk.assign
            CT, cn, moved2 = km_centers(blk.S, blk.Wq, CT, K, self.k, self.kw, self.measure, threads=self.threads)
            it += 1
            if not until_stable and float(moved2.max()) <= tol * tol:       # the iteration's one small read
                break
        return CT, cn, it


def _weighted_pick(weights: np.ndarray, u: float) -> int:
    """The first index whose running weight sum exceeds ``u`` times the total (sequential fp64 sums)."""
    cum = np.cumsum(weights)
    j = int(np.searchsorted(cum, u * cum[-1], side="right"))
    return min(j, len(weights) - 1)


def _local_kmeans(cand: _Rows, cw: np.ndarray, k: int, measure: str, seed: int, F: int, vmax: float, xnmax: float,
                  dev, threads: int) -> tuple:
    """Spark's LocalKMeans on the candidate rows themselves (a small CSR with the candidate
    weights): weighted k-means++ and at most ``LOCAL_ITERATIONS`` Lloyd iterations. Returns ``(CT, cn)``."""
    m = len(cand)
    pos = np.maximum(cw, 0.0)
    sel = pos > 0 if np.count_nonzero(pos > 0) >= k else np.ones(m, dtype=bool)
    if not sel.all():                                  # a pass needs weights > 0: rows nothing is closest to leave
        keep = np.nonzero(sel)[0]
        cand, cw, m = _Rows([cand.gidx[i] for i in keep], [cand.idx[i] for i in keep], [cand.val[i] for i in keep]), \
            cw[keep], len(keep)
    cw = np.where(cw > 0, cw, 1.0)
    prob = _Problem(cand.column(F, dev), torch.from_numpy(cw).to(dev), measure, float(cw.max()), vmax, xnmax, m,
                    hot=[], threads=threads)
    u = hash_uniform(seed, _STAGE_LOCAL, torch.arange(k, dtype=torch.int64)).numpy()
    cs = _Centers(F, k, measure, dev)
    chosen = [_weighted_pick(cw, float(u[0]))]
    cs.fill(cand.idx[chosen[0]], cand.val[chosen[0]])            # the columns not drawn yet repeat the first center
    for c in range(1, k):
        d = prob.step(cs, k, sums=False, want_rows=True).dist.cpu().numpy()
        cost = cw * d
        cost[chosen] = 0.0
        if not cost.sum() > 0:                         # every candidate is a center already
            j = next(i for i in range(m) if i not in chosen)
        else:
            j = _weighted_pick(cost, float(u[c]))
        chosen.append(j)
        cs.set(c, cand.idx[j], cand.val[j])
    CT, cn, _ = prob.lloyd(cs.CT, cs.cn, k, LOCAL_ITERATIONS, 0.0, until_stable=True)
    return CT, cn


def _dp_sum(t: torch.Tensor) -> torch.Tensor:
    return D.all_reduce_sum(t) if D.is_dist() else t


def _init_random(prob: _Problem, k: int, seed: int, offset: int, n: int) -> _Rows:
    """The ``k`` rows with the smallest priorities over all ranks, ties to the smaller row."""
    g = torch.arange(offset, offset + n, dtype=torch.int64)
    u = hash_uniform(seed, _STAGE_RANDOM, g)
    local = torch.sort(torch.sort(u, stable=True).indices[:k]).values
    rows = _gather_rows(prob.vc, local, offset, prob.dev)
    pri = hash_uniform(seed, _STAGE_RANDOM, torch.tensor(rows.gidx, dtype=torch.int64)).numpy()
    order = np.lexsort((np.asarray(rows.gidx), pri))[:k]
    return _Rows([rows.gidx[i] for i in order], [rows.idx[i] for i in order], [rows.val[i] for i in order])


def _init_parallel(prob: _Problem, k: int, steps: int, seed: int, offset: int, n: int) -> tuple:
    """Spark's k-means||: ``(candidates, their weights)``, the candidates distinct and in the order
    they were drawn."""
    g = torch.arange(offset, offset + n, dtype=torch.int64)
    u0 = hash_uniform(seed, _STAGE_FIRST, g)
    first = _gather_rows(prob.vc, torch.sort(u0, stable=True).indices[:1], offset, prob.dev)
    pri = hash_uniform(seed, _STAGE_FIRST, torch.tensor(first.gidx, dtype=torch.int64)).numpy()
    j = int(np.lexsort((np.asarray(first.gidx), pri))[0])
    cand = _Rows([first.gidx[j]], [first.idx[j]], [first.val[j]])
    w = prob.w.cpu().numpy() if prob.w is not None else np.ones(n)
    best = prob.nearest(cand)
    for r in range(int(steps)):
        d = best[0]
        wd = d if prob.w is None else prob.w * d
        costq = int(_dp_sum(torch.round(wd * float(2 ** prob.kc)).to(torch.int64).sum().reshape(1))[0])
        if costq <= 0:
            break
        cost = math.ldexp(float(costq), -prob.kc)
        u = hash_uniform(seed, _STAGE_ROUND + r, g).numpy()
        keep = u < ((2.0 * k) * w) * d.cpu().numpy() / cost
        new = _gather_rows(prob.vc, torch.from_numpy(np.nonzero(keep)[0]), offset, prob.dev)
        if len(new):
            best = prob.nearest(new, best, base=len(cand))
            cand.extend(new)
    # weights: the weight sums of the rows closest to each candidate, exact in fixed point
    ones = torch.ones(n, dtype=torch.float64, device=prob.dev)
    q = torch.round((prob.w if prob.w is not None else ones) * float(2 ** prob.kw)).to(torch.int64)
    wq = _dp_sum(torch.zeros(len(cand), dtype=torch.int64, device=prob.dev).index_add_(0, best[1], q)).cpu().numpy()
    cw = np.ldexp(wq.astype(np.float64), -prob.kw)
    seen, out, weights = {}, _Rows(), []
    for i in range(len(cand)):
        key = (cand.idx[i].tobytes(), cand.val[i].astype(np.float64).tobytes())
        if key in seen:
            weights[seen[key]] += cw[i]
            continue
        seen[key] = len(out)
        out.extend(_Rows([cand.gidx[i]], [cand.idx[i]], [cand.val[i]]))
        weights.append(cw[i])
    return out, np.asarray(weights, dtype=np.float64)


def fit_kmeans(features, k: int, weights=None, max_iter: int = 20, tol: float = 1e-4, init_mode: str = "k-means||",
               init_steps: int = 2, distance_measure: str = "euclidean", seed: int = -1689246527, device=None,
               hot=None, threads: int = 0) -> dict:
    """Fit on a ``VectorColumn`` (rows of this rank under data parallelism). Returns ``centers``
    [K, F] (``K <= k``: fewer distinct candidates give fewer centers, as in Spark), ``init_centers``
    [K, F], ``k`` = K, ``F``, ``cost`` and ``costq`` (the weighted cost of the final centers, and its
    exact fixed-point sum), ``sizes`` [K] (rows per cluster), ``num_iter`` and the scale exponents
    ``ek`` / ``ekw`` / ``ekc``."""
    lim = km_limits()
    k = int(k)
    if not 2 <= k <= lim["max_k"]:
        raise ValueError(f"KMeans supports k in 2 .. {lim['max_k']}, got {k}")
    if init_mode not in INIT_MODES:
        raise ValueError(f"unknown KMeans initMode {init_mode!r} (random, k-means||)")
    if distance_measure not in MEASURES:
        raise ValueError(f"unknown KMeans distanceMeasure {distance_measure!r} (euclidean, cosine)")
    if int(max_iter) < 0 or not float(tol) >= 0.0 or int(init_steps) < 1:
        raise ValueError("KMeans needs maxIter >= 0, tol >= 0 and initSteps >= 1")
    vc0 = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    dev, vc, _, w, n = coerce_rows(vc0, torch.zeros(len(vc0), dtype=torch.float64), weights, device)
    indptr, idx, val = _csr(vc)
    vc = VectorColumn(vc.size, indptr, idx, val)
    F = int(vc.size)
    zero, one = torch.zeros((), dtype=torch.float64, device=dev), torch.ones((), dtype=torch.float64, device=dev)
    # (largest weight, largest |value|, largest row norm)
    (wmax, vmax, nmax), n_global = reduce_statistics(
        [w.max() if w is not None and n else one, val.abs().max().to(torch.float64) if val.numel() else zero,
         sim_norms(indptr, val).max() if n else zero], n, dev)
    if not math.isfinite(wmax) or wmax <= 0:
        raise ValueError("KMeans weights must be finite and > 0")
    if not math.isfinite(vmax) or not math.isfinite(nmax * nmax):
        raise ValueError("KMeans requires finite feature values")
    offset = 0
    if D.is_dist():
        counts = D.all_gather(torch.tensor([n], dtype=torch.int64, device=dev)).view(-1).tolist()
        offset = int(sum(counts[:D.rank()]))
    prob = _Problem(vc, w, distance_measure, wmax, vmax, nmax * nmax, n_global, hot=hot, threads=threads)

    # bad input raises on every rank, before anything is drawn
    probe = _Centers(F, 2, distance_measure, dev)
    flag = torch.tensor([prob.step(probe, 2, sums=False, want_rows=False).flag if n else 0], dtype=torch.int64, device=dev)
    if int(D.all_reduce_max(flag)[0] if D.is_dist() else flag[0]):
        _raise_bad_input("km", idx, val, None, w, F)
        raise ValueError("KMeans: bad input on another rank")
    if n_global < 2:
        raise ValueError("KMeans needs at least two rows")

    seed = int(seed)
    if init_mode == "random":
        rows = _init_random(prob, k, seed, offset, n)
        if len(rows) < 2:
            raise ValueError("KMeans needs at least two initial centers")
        cs = _Centers.of_rows(rows, F, distance_measure, dev)
        CT, cn, K = cs.CT, cs.cn, len(rows)
    else:
        cand, cw = _init_parallel(prob, k, int(init_steps), seed, offset, n)
        if len(cand) < 2:
            raise ValueError("KMeans found fewer than two distinct initial centers")
        if len(cand) <= k:
            cs = _Centers.of_rows(cand, F, distance_measure, dev)
            CT, cn, K = cs.CT, cs.cn, len(cand)
        else:
            CT, cn = _local_kmeans(cand, cw, k, distance_measure, seed, F, vmax, nmax * nmax, dev, threads)
            K = k
    init_centers = CT[:, :K].t().contiguous().cpu().numpy()

    CT, cn, num_iter = prob.lloyd(CT, cn, K, int(max_iter), float(tol))
    tail = _dp_sum(prob.step((CT, cn), K, sums=False, want_rows=False).block).cpu().numpy()
    costq = int(tail[2 * K])
    return {"centers": CT[:, :K].t().contiguous().cpu().numpy(), "init_centers": init_centers, "k": K, "F": F,
            "cost": math.ldexp(float(costq), -prob.kc), "costq": costq, "sizes": tail[K:2 * K].copy(),
            "num_iter": num_iter, "ek": prob.k, "ekw": prob.kw, "ekc": prob.kc, "measure": distance_measure}


def predict_kmeans(features, centers: np.ndarray, distance_measure: str = "euclidean", device=None,
                   threads: int = 0) -> torch.Tensor:
    """The cluster of every row, int32 on the column's device: the assign-only pass against the
    centers (``centers`` [K, F]; cosine centers have norm 1). Raises ``ValueError`` for bad input."""
    vc = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    if device is not None:
        vc = vc.to(torch.device(device))
    centers = np.asarray(centers, dtype=np.float64)
    K, F = centers.shape
    if vc.size != F:
        raise ValueError(f"features have size {vc.size}, the model expects {F}")
    dev = vc.device
    CT = torch.zeros((F, km_padded(K)), dtype=torch.float64, device=dev)
    CT[:, :K] = torch.from_numpy(np.ascontiguousarray(centers.T)).to(dev)
    cn = torch.zeros(km_padded(K), dtype=torch.float64, device=dev)
    cn[:K] = torch.from_numpy(np.array([math.fsum(c * c) for c in centers])).to(dev)
    return km_step(vc, CT, cn, K, distance_measure, 0, 0, 0, sums=False, want_rows=True, threads=threads).assign
