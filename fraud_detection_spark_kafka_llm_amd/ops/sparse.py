"""Sparse ops over ``VectorColumn`` CSR data (native: ``csrc/sparse_kernels.hip`` / ``sparse_cpu.cpp``)."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import native
from .text import ClassLinearScorer, LinearScorer, TreeArrays, TreePaths


def _csr(vc):
    indptr, idx, val = vc.csr()
    if val.dtype not in (torch.float32, torch.float64):
        val = val.to(torch.float64)
    return indptr.contiguous(), idx.to(torch.int32).contiguous(), val.contiguous()


def score_csr(vc, scorer, threads: int = 0) -> torch.Tensor:
    """Raw scores ``[N, K]`` fp64: LR margin (K=1) or tree-ensemble sums (K = leaf width)."""
    indptr, idx, val = _csr(vc)
    dev = indptr.device
    n = indptr.numel() - 1
    C = native.lib()
    if isinstance(scorer, LinearScorer):
        if scorer.w.size > vc.size:
            raise ValueError("coefficient vector longer than the feature space")
        out = torch.empty((n, 1), dtype=torch.float64, device=dev)
        w = scorer.weights(dev)
        if w.numel() < vc.size:   # features beyond the model's width contribute nothing
            w = torch.cat([w, torch.zeros(vc.size - w.numel(), dtype=torch.float64, device=dev)])
        C.score_csr(indptr, idx, val, w, scorer.b, None, 1, False, out, threads)
        return out
    if isinstance(scorer, TreeArrays):
        if scorer.max_feature() >= vc.size:
            raise ValueError("tree references a feature beyond the feature space")
        out = torch.empty((n, scorer.K), dtype=torch.float64, device=dev)
        C.score_csr(indptr, idx, val, None, 0.0, scorer.tensors(dev), scorer.K, scorer.cmp_less, out, threads)
        return out
    if isinstance(scorer, ClassLinearScorer):
        if scorer.W.shape[0] > vc.size:
            raise ValueError("coefficient matrix longer than the feature space")
        W, b = scorer.tensors(dev, vc.size)
        out = torch.empty((n, scorer.num_classes), dtype=torch.float64, device=dev)
        C.nb_score(indptr, idx, val, W, b, out, threads)
        return out
    raise TypeError(f"unknown scorer {type(scorer)}")


def contrib_limits() -> dict:
    """Structural constants of the TreeSHAP kernels (block size of the summation order, paths per
    workgroup chunk, rows per workgroup and per launch tile, depth limit)."""
    return dict(native.lib().contrib_limits())


def tree_contributions(vc, paths, threads: int = 0) -> torch.Tensor:
    """Path-dependent TreeSHAP of every row: ``[N, U]`` fp64, column ``u`` = contribution of feature
    ``paths.features[u]`` to the explained output; a row sums to its score minus ``paths.bias``.
    Rows hold finite values with distinct indices. The device path runs in tiles of
    ``rows_per_tile`` rows so its scratch stays bounded; device and host agree bitwise."""
    if not isinstance(paths, TreePaths):
        raise TypeError(f"expected TreePaths, got {type(paths)}")
    if paths.max_feature() >= vc.size:
        raise ValueError("tree references a feature beyond the feature space")
    indptr, idx, val = _csr(vc)
    dev = indptr.device
    n = indptr.numel() - 1
    U = int(paths.features.size)
    out = torch.empty((n, U), dtype=torch.float64, device=dev)
    if n == 0 or U == 0:
        return out
    C = native.lib()
    tabs = paths.tensors(dev)
    if dev.type != "cuda":
        C.tree_contributions(indptr, idx, val, tabs, paths.cmp_less, out, None, threads)
        return out
    tile = int(C.contrib_limits()["rows_per_tile"])
    xs = torch.empty(U * tile, dtype=torch.float64, device=dev)
    masks = torch.empty(paths.num_paths * tile, dtype=torch.int32, device=dev)
    partials = torch.empty(paths.num_blocks * tile, dtype=torch.float64, device=dev)
    for r0 in range(0, n, tile):
        r1 = min(n, r0 + tile)
        xs.zero_()
        C.tree_contributions(indptr[r0:r1 + 1], idx, val, tabs, paths.cmp_less, out[r0:r1], [xs, masks, partials], 0)
    return out


def spmv(indptr, idx, val, x: torch.Tensor, threads: int = 0) -> torch.Tensor:
    y = torch.empty(indptr.numel() - 1, dtype=torch.float64, device=indptr.device)
    native.lib().spmv(indptr, idx, val, x, y, threads)
    return y


def spmv_t(indptr, idx, val, r: torch.Tensor, cols: int, threads: int = 0) -> torch.Tensor:
    g = torch.zeros(cols, dtype=torch.float64, device=indptr.device)
    native.lib().spmv_t(indptr, idx, val, r, g, threads)
    return g


def lr_limits() -> dict:
    """Structural constants of the logistic-regression kernels (rows per partial of ``lr_forward``,
    width of the reducer, workgroup size and workgroup cap of the parameter passes)."""
    return dict(native.lib().lr_limits())


def lr_reduce(partials: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sums of the rows of ``partials`` [K, P] in the reducer's fixed order (it depends on P alone)."""
    if out is None:
        out = torch.empty(partials.shape[0], dtype=torch.float64, device=partials.device)
    native.lib().lr_reduce(partials, out)
    return out


def lr_forward(indptr, idx, val, xs: torch.Tensor, b: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
               want_rows: bool = False, out: Optional[torch.Tensor] = None, threads: int = 0):
    """Fused evaluation of binary logistic regression over a CSR: margins ``X xs + b`` (bitwise
    ``spmv(...) + b``), residuals ``r = w (sigma(m) - y)`` and the sums ``(sum w loss, sum r)``, written
    to ``out`` [2] when given. Returns ``(r, sums)``, or ``(r, sums, loss_row, margin)`` with
    ``want_rows``. ``b`` is a one-element tensor on the CSR's device."""
    dev = indptr.device
    n = indptr.numel() - 1
    C = native.lib()
    per = int(C.lr_limits()["rows_per_partial"])
    partials = torch.empty((2, (n + per - 1) // per), dtype=torch.float64, device=dev)
    r = torch.empty(n, dtype=torch.float64, device=dev)
    loss_row = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    margin = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    C.lr_forward(indptr, idx, val, xs, b, y, w, r, loss_row, margin, partials, threads)
    sums = lr_reduce(partials, out)
    return (r, sums, loss_row, margin) if want_rows else (r, sums)


def lr_owlqn_step(x: torch.Tensor, d: torch.Tensor, xi: torch.Tensor, pg: torch.Tensor, scale: torch.Tensor,
                  t: float, threads: int = 0):
    """OWL-QN trial point over ``F + 1`` parameters (the last is the intercept, never projected):
    ``x_new = pi(x + t d; xi)`` with coefficients that leave their orthant set to exactly 0.0 and
    ``xs_new = scale * x_new[:F]``. Returns ``(x_new, xs_new, sums)`` with
    ``sums = (|x_new[:F]|_1, x_new[:F] . x_new[:F], pg . (x_new - x))``."""
    C = native.lib()
    n = x.numel()
    x_new = torch.empty_like(x)
    xs_new = torch.empty(n - 1, dtype=torch.float64, device=x.device)
    partials = torch.empty((3, int(C.lr_param_groups(n))), dtype=torch.float64, device=x.device)
    C.lr_owlqn_step(x, d, xi, pg, scale, float(t), x_new, xs_new, partials, threads)
    return x_new, xs_new, lr_reduce(partials)


def lr_pseudo_grad(parts: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, wsum: float, l1: float, l2: float,
                   fit_intercept: bool = True, threads: int = 0):
    """Gradient pass over ``F + 1`` parameters from ``parts = (sum w loss, sum r, X^T r)`` [F + 2]:
    the smooth gradient ``g = scale X^T r / W + l2 beta`` (intercept: ``sum r / W``), the
    pseudo-gradient ``pg`` of ``l1 |beta|_1`` and the orthant ``xi``. Returns ``(g, pg, xi, |pg|^2)``."""
    C = native.lib()
    n = x.numel()
    g, pg, xi = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    partials = torch.empty((1, int(C.lr_param_groups(n))), dtype=torch.float64, device=x.device)
    C.lr_pseudo_grad(parts, scale, x, float(wsum), float(l1), float(l2), bool(fit_intercept), g, pg, xi, partials,
                     threads)
    return g, pg, xi, lr_reduce(partials)


def nb_limits() -> dict:
    """Structural constants of the Naive Bayes kernels: ``max_classes``, the default rows of a
    workgroup (``chunk_rows``), the default and the largest LDS table of the hot features
    (``table_bytes``, ``max_table_bytes``; a class holds ``bytes // (8 C)`` slots), the largest scale
    exponent ``k_max``, ``sum_bits`` (``|S| < 2^sum_bits``), the rows whose document frequencies choose
    the default hot set (``prefix_rows``), wave and workgroup size."""
    return dict(native.lib().nb_limits())


def nb_scale_exponent(tmax: float, n_rows: int) -> int:
    """``k = min(k_max, sum_bits - n_rows.bit_length() - e)`` with ``max(tmax, 1.0) < 2^e`` (``frexp``);
    raises ``ValueError`` when ``k < 0`` (the exact sums would not fit 2^sum_bits)."""
    lim = nb_limits()
    tmax = float(tmax)
    if not math.isfinite(tmax) or tmax < 0:
        raise ValueError(f"Naive Bayes needs finite, non-negative values and weights (largest term {tmax})")
    e = math.frexp(max(tmax, 1.0))[1]
    k = min(int(lim["k_max"]), int(lim["sum_bits"]) - int(n_rows).bit_length() - e)
    if k < 0:
        raise ValueError(f"terms up to {tmax:g} over {n_rows} rows do not fit the exact {lim['sum_bits']}-bit sums")
    return k


def nb_hot_set(indptr, idx, val, size: int, num_classes: int, table_bytes: int = 0) -> torch.Tensor:
    """Default hot set of ``nb_sums``: the ``table_bytes // (8 C)`` most frequent features of the
    first ``prefix_rows`` rows (features that occur there at all), as int32 feature ids."""
    lim = nb_limits()
    slots = int(table_bytes or lim["table_bytes"]) // (8 * int(num_classes))
    rows = min(int(indptr.numel()) - 1, int(lim["prefix_rows"]))
    if slots <= 0 or rows <= 0:
        return torch.zeros(0, dtype=torch.int32, device=idx.device)
    end = int(indptr[rows])
    df = doc_freq(idx[:end], val[:end], size)
    top = torch.topk(df, min(slots, size))
    return top.indices[top.values > 0].to(torch.int32)


def nb_hot_tables(hot_feat: torch.Tensor, size: int, num_classes: int) -> tuple:
    """``(slot_of int16 [F], hot_feat int32 [H])`` of a hot set for the device pass (``slot_of`` is read
    as uint16: -1 = 0xFFFF = not hot), or ``(None, None)`` for an empty one."""
    if hot_feat.numel() * 8 * int(num_classes) > nb_limits()["max_table_bytes"]:
        raise ValueError("the hot set exceeds the LDS table")
    if hot_feat.numel() == 0:
        return None, None
    if int(hot_feat.min()) < 0 or int(hot_feat.max()) >= size:
        raise ValueError("hot feature outside the feature space")
    slot_of = torch.full((size,), -1, dtype=torch.int16, device=hot_feat.device)
    slot_of[hot_feat.to(torch.int64)] = torch.arange(hot_feat.numel(), dtype=torch.int16, device=hot_feat.device)
    return slot_of, hot_feat.to(torch.int32).contiguous()


def hot_tables(indptr, idx, val, size: int, num_classes: int, hot=None) -> tuple:
    """``nb_hot_tables`` of ``hot`` (feature ids; ``None`` = ``nb_hot_set``) for a CSR on a HIP device,
    ``(None, None)`` on the host, which has no hot set."""
    if indptr.device.type != "cuda":
        return None, None
    hot_feat = nb_hot_set(indptr, idx, val, size, num_classes) if hot is None else \
        torch.as_tensor(hot, dtype=torch.int32, device=indptr.device).reshape(-1)
    return nb_hot_tables(hot_feat, size, num_classes)


def nb_sums(vc, labels, weights, num_classes: int, k: int, kw: int, bernoulli: bool = False, hot=None,
            threads: int = 0, chunk_rows: int = 0):
    """Exact class-conditional sums of a CSR column for Naive Bayes, ``(S [C, F], Wq [C], cnt [C])``
    int64: ``S[c, f] = sum rint(w_i x_ij 2^k)`` over the stored entries ``f`` of the rows of class
    ``c``, ``Wq[c] = sum rint(w_i 2^kw)``, ``cnt[c]`` the rows of class ``c``. Integer sums do not depend
    on order: ``hot`` (device: feature ids accumulated in LDS; ``None`` = ``nb_hot_set``, empty =
    every entry goes to a global atomic), ``chunk_rows`` and ``threads`` change the speed only.
    Raises ``ValueError`` for a label that is no integer in ``0 .. C - 1``, a weight that is not
    finite and > 0, and a value that is negative or not finite (Bernoulli: not 0 or 1)."""
    lim = nb_limits()
    C_ = int(num_classes)
    if not 2 <= C_ <= lim["max_classes"]:
        raise ValueError(f"Naive Bayes supports 2 .. {lim['max_classes']} classes, got {C_}")
    indptr, idx, val = _csr(vc)
    dev, F = indptr.device, int(vc.size)
    y = torch.as_tensor(labels).to(device=dev, dtype=torch.float64).contiguous()
    w = None if weights is None else torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
    slot_of, hot_feat = hot_tables(indptr, idx, val, F, C_, hot)
    out = torch.zeros(C_ * F + 2 * C_ + 1, dtype=torch.int64, device=dev)
    native.lib().nb_sums(indptr, idx, val, y, w, C_, F, int(k), int(kw), bool(bernoulli), slot_of, hot_feat, out,
                         int(chunk_rows), threads)
    host = out.cpu()                                   # the flag travels with the sums
    if int(host[-1]):
        _raise_bad_input("nb", idx, val, y, w, F, C_, bool(bernoulli))
    S = host[:C_ * F].view(C_, F)
    return S, host[C_ * F:C_ * F + C_], host[C_ * F + C_:C_ * F + 2 * C_]


# family -> (its name in messages, whether a weight may be 0)
_FAMILIES = {"nb": ("Naive Bayes", False), "mlr": ("multinomial logistic regression", True),
             "svc": ("LinearSVC", True), "km": ("KMeans", False)}


def _raise_bad_input(family: str, idx, val, y, w, F: int, C_: Optional[int] = None, bernoulli: bool = False) -> None:
    """Name the bad input behind a pass's flag word (the slow path: only taken on an error). Labels
    are integers in ``0 .. C_ - 1``, or 0 / 1 where ``C_`` is ``None``; ``y`` is ``None`` for a family
    without labels (KMeans)."""
    name, zero_ok = _FAMILIES[family]
    labels_ok = None if y is None else \
        (y == 0) | (y == 1) if C_ is None else (y >= 0) & (y < C_) & (y == torch.floor(y))
    if labels_ok is not None and not bool(torch.all(labels_ok)):
        raise ValueError(f"{name} labels must be " + ("0 or 1" if C_ is None else f"integers in 0 .. {C_ - 1}"))
    if w is not None and not bool(torch.all(torch.isfinite(w) & ((w >= 0) if zero_ok else (w > 0)))):
        raise ValueError(f"{name} weights must be finite and " + (">= 0" if zero_ok else "> 0"))
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= F):
        raise ValueError("feature index outside the feature space")
    if family == "km" and bool(torch.all(torch.isfinite(val))):
        raise ValueError("KMeans requires rows of a finite norm that is not zero under the cosine measure")
    if family != "nb":
        raise ValueError(f"{name} requires finite feature values")
    if bernoulli:
        raise ValueError("Bernoulli Naive Bayes requires feature values 0 or 1")
    raise ValueError("Multinomial Naive Bayes requires finite, non-negative feature values")


# ---------------------------------------------------------------------------------------------- KMeans
KM_MEASURES = {"euclidean": 0, "cosine": 1}


def km_limits() -> dict:
    """Structural constants of the KMeans kernels: ``max_k``, the centers of a register ``tile``, the
    width of ``km_centers``' summation tree (``centers_block``) and those of ``nb_limits`` it shares
    (``chunk_rows``, ``table_bytes``, ``k_max``, ``sum_bits``, ``prefix_rows``, wave and workgroup
    size); ``max_table_bytes`` is its own, the table shares the workgroup with ``2 max_k + 1`` sums."""
    return dict(native.lib().km_limits())


def km_padded(K: int) -> int:
    """``Kp``: ``K`` rounded up to the tile."""
    tile = int(km_limits()["tile"])
    return (int(K) + tile - 1) // tile * tile


def _km_check(name: str, K: int, measure: str) -> int:
    lim = km_limits()
    if not 2 <= int(K) <= lim["max_k"]:
        raise ValueError(f"{name}: KMeans passes take 2 .. {lim['max_k']} centers, got {K}")
    if measure not in KM_MEASURES:
        raise ValueError(f"{name}: unknown distance measure {measure!r} (euclidean, cosine)")
    return KM_MEASURES[measure]


@dataclass
class KmBlock:
    """The int64 block of one ``km_step``: ``S`` [K, F] (``None`` for an assign-only pass), ``Wq`` [K],
    ``cnt`` [K], ``costq``, the flag word, and the per-row outputs when they were asked for. The block
    stays on the CSR's device."""
    block: torch.Tensor
    F: int
    K: int
    sums: bool
    assign: Optional[torch.Tensor] = None
    dist: Optional[torch.Tensor] = None

    @property
    def _base(self) -> int:
        return self.K * self.F if self.sums else 0

    @property
    def S(self) -> Optional[torch.Tensor]:
        return self.block[:self._base].view(self.K, self.F) if self.sums else None

    @property
    def Wq(self) -> torch.Tensor:
        return self.block[self._base:self._base + self.K]

    @property
    def cnt(self) -> torch.Tensor:
        return self.block[self._base + self.K:self._base + 2 * self.K]

    @property
    def costq(self) -> int:
        return int(self.block[-2])

    @property
    def flag(self) -> int:
        return int(self.block[-1])


def km_step(vc, CT: torch.Tensor, cn: torch.Tensor, K: int, measure: str, k: int, kw: int, kc: int, weights=None,
            hot=None, sums: bool = True, want_rows: bool = False, chunk_rows: int = 0, threads: int = 0,
            check: bool = True) -> KmBlock:
    """One Lloyd evaluation of a CSR column against ``K`` centers (``CT`` [F, Kp] fp64 feature-major,
    padding columns zero; ``cn`` [Kp] their squared norms) in one fused pass: every row's distances
    (dots and the squared norm in spmv's order), its cluster ``a`` (the smallest index that attains
    the least distance) and the exact int64 sums ``S[a, f] += rint(s x 2^k)`` (``s = w``, cosine:
    ``w / |x|``), ``Wq[a] += rint(w 2^kw)``, ``cnt[a] += 1``, ``costq += rint(w d_a 2^kc)``.
    ``sums=False`` skips ``S`` (assign only); ``want_rows`` adds ``assign`` int32 and ``dist`` fp64 per
    row. Integer sums do not depend on order: ``hot`` (device: feature ids accumulated in LDS; ``None``
    = ``nb_hot_set``, empty = every entry goes to a global atomic; a pair is taken as ready
    ``nb_hot_tables``), ``chunk_rows`` and ``threads`` change the speed only. Raises ``ValueError``
    before any launch for ``K`` outside ``2 .. max_k``, an unknown measure or a shape mismatch, and
    with ``check`` after the pass for bad input (a feature id outside the space, a value or a row norm
    that is not finite, a weight that is not finite and > 0, a zero row under cosine); without
    ``check`` the caller tests ``flag``."""
    m = _km_check("km_step", K, measure)
    lim = km_limits()
    K, Kp = int(K), km_padded(K)
    indptr, idx, val = _csr(vc)
    dev, F, n = indptr.device, int(vc.size), indptr.numel() - 1
    if CT.dtype != torch.float64 or CT.dim() != 2 or tuple(CT.shape) != (F, Kp) or CT.device != dev:
        raise ValueError(f"km_step: CT is float64 [{F}, {Kp}] on the CSR's device")
    if cn.dtype != torch.float64 or cn.numel() != Kp or cn.device != dev:
        raise ValueError(f"km_step: cn is float64 [{Kp}] on the CSR's device")
    if not all(0 <= int(e) <= lim["k_max"] for e in (k, kw, kc)):
        raise ValueError(f"km_step: scale exponents lie in 0 .. {lim['k_max']}")
    w = None if weights is None else torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
    if w is not None and w.numel() != n:
        raise ValueError("km_step: weights needs one entry per row")
    slot_of = hot_feat = None
    if sums and dev.type == "cuda":
        slot_of, hot_feat = hot if isinstance(hot, tuple) else hot_tables(indptr, idx, val, F, K, hot)
        if hot_feat is not None and hot_feat.numel() * 8 * K > lim["max_table_bytes"]:
            raise ValueError("km_step: the hot set exceeds the LDS table")
    out = torch.zeros((K * F if sums else 0) + 2 * K + 2, dtype=torch.int64, device=dev)
    assign = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
    dist = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    native.lib().km_step(indptr, idx, val, w, CT.contiguous(), cn.contiguous(), K, m, int(k), int(kw), int(kc),
                         slot_of, hot_feat, out, bool(sums), assign, dist, int(chunk_rows), threads)
    blk = KmBlock(out, F, K, bool(sums), assign, dist)
    if check and blk.flag:
        _raise_bad_input("km", idx, val, None, w, F)
    return blk


def km_centers(S: torch.Tensor, Wq: torch.Tensor, CT_old: torch.Tensor, K: int, k: int, kw: int, measure: str,
               threads: int = 0) -> tuple:
    """The update of a Lloyd iteration on the sums' device, ``(CT [F, Kp], cn [Kp], moved2 [K])``:
    ``center_c = S[c] 2^-k / (Wq[c] 2^-kw)`` (cosine: divided by its norm), a cluster with ``Wq[c] = 0``
    keeps its center; ``cn`` the squared norms and ``moved2`` the squared moves, every sum over the
    features in an order that depends on ``F`` alone (bitwise equal on host and device). Raises
    ``ValueError`` before any launch for ``K`` outside ``2 .. max_k``, an unknown measure or a shape
    mismatch."""
    m = _km_check("km_centers", K, measure)
    K, Kp = int(K), km_padded(K)
    dev = S.device
    if CT_old.dim() != 2 or CT_old.shape[1] != Kp or CT_old.dtype != torch.float64 or CT_old.device != dev:
        raise ValueError(f"km_centers: CT_old is float64 [F, {Kp}] on the sums' device")
    F = int(CT_old.shape[0])
    if S.dtype != torch.int64 or S.numel() != K * F or Wq.dtype != torch.int64 or Wq.numel() != K or Wq.device != dev:
        raise ValueError(f"km_centers: S is int64 [{K}, {F}], Wq int64 [{K}]")
    CT = torch.zeros((F, Kp), dtype=torch.float64, device=dev)
    cn = torch.zeros(Kp, dtype=torch.float64, device=dev)
    moved2 = torch.zeros(K, dtype=torch.float64, device=dev)
    native.lib().km_centers(S.contiguous(), Wq.contiguous(), CT_old.contiguous(), K, int(k), int(kw), m, CT, cn, moved2,
                            threads)
    return CT, cn, moved2


# ---------------------------------------------------------------------------------------------- bisecting / silhouette
def clu_limits() -> dict:
    """Structural constants of ``km_group_step`` and ``sil_score``: ``max_k``, ``max_width`` (the
    candidates of a row), the ``tile`` and those of ``km_limits`` they share (``chunk_rows``,
    ``table_bytes``, ``max_table_bytes``, ``k_max``, ``sum_bits``, wave and workgroup size)."""
    return dict(native.lib().clu_limits())


def _clu_measure(name: str, measure: str) -> int:
    if measure not in KM_MEASURES:
        raise ValueError(f"{name}: unknown distance measure {measure!r} (euclidean, cosine)")
    return KM_MEASURES[measure]


def _clu_rows(name: str, what: str, t, n: int, dev) -> torch.Tensor:
    """An int32 entry per row on the CSR's device."""
    t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.numel() != n:
        raise ValueError(f"{name}: {what} is an integer per row")
    return t.to(device=dev, dtype=torch.int32).contiguous().view(-1)


@dataclass
class KmGroupBlock:
    """The int64 block of one ``km_group_step``: ``S`` [K, F] (``None`` for an assign-only pass), ``Wq``
    [K], ``cnt`` [K], ``costq`` [K] (per cluster), the flag word, and the per-row outputs when they
    were asked for. The block stays on the CSR's device."""
    block: torch.Tensor
    F: int
    K: int
    sums: bool
    assign: Optional[torch.Tensor] = None
    dist: Optional[torch.Tensor] = None

    @property
    def _base(self) -> int:
        return self.K * self.F if self.sums else 0

    @property
    def S(self) -> Optional[torch.Tensor]:
        return self.block[:self._base].view(self.K, self.F) if self.sums else None

    @property
    def Wq(self) -> torch.Tensor:
        return self.block[self._base:self._base + self.K]

    @property
    def cnt(self) -> torch.Tensor:
        return self.block[self._base + self.K:self._base + 2 * self.K]

    @property
    def costq(self) -> torch.Tensor:
        return self.block[self._base + 2 * self.K:self._base + 3 * self.K]

    @property
    def flag(self) -> int:
        return int(self.block[-1])


def km_group_step(vc, group, W: int, G: int, CT: torch.Tensor, cn: torch.Tensor, measure: str, k: int, kw: int,
                  kc: int, weights=None, hot=None, sums: bool = True, want_rows: bool = False, chunk_rows: int = 0,
                  threads: int = 0, check: bool = True) -> KmGroupBlock:
    """A Lloyd step in which the caller names each row's candidates: row ``r`` with ``g = group[r]``
    competes among the ``W`` (1 or 2) adjacent centers ``W g .. W g + W - 1`` of ``CT`` [F, Kp] (``K =
    max(2, W G) <= max_k``, ``Kp = km_padded(K)``, ``cn`` [Kp] the squared norms). ``g < 0`` skips the row:
    only ``group[r]`` is read, nothing is added, ``assign = -1`` and ``dist = 0``. One walk in spmv's
    order gives the squared norm and the dots, ``d_i = km_distance``, the left child wins ties, and
    the exact int64 sums go to the cluster ``c = W g + a``: ``S[c, f] += rint(s x 2^k)``, ``Wq[c] +=
    rint(w 2^kw)``, ``cnt[c] += 1`` and the per-cluster ``costq[c] += rint(w d 2^kc)``. ``sums``,
    ``want_rows``, ``hot``, ``chunk_rows``, ``threads`` and ``check`` as in ``km_step``: they change no
    bit. Raises ``ValueError`` before any launch for a width outside 1 .. 2, ``W G > max_k``, an
    unknown measure or a shape mismatch, and with ``check`` after the pass for bad input
    (``km_step``'s cases and a group ``>= G``)."""
    name = "km_group_step"
    lim = clu_limits()
    W, G = int(W), int(G)
    if W not in (1, 2) or G < 1 or W * G > lim["max_k"]:
        raise ValueError(f"{name}: the width is 1 or 2 and width * groups at most {lim['max_k']}, got {W} x {G}")
    m = _clu_measure(name, measure)
    K = max(2, W * G)
    Kp = km_padded(K)
    indptr, idx, val = _csr(vc)
    dev, F, n = indptr.device, int(vc.size), indptr.numel() - 1
    if CT.dtype != torch.float64 or CT.dim() != 2 or tuple(CT.shape) != (F, Kp) or CT.device != dev:
        raise ValueError(f"{name}: CT is float64 [{F}, {Kp}] on the CSR's device")
    if cn.dtype != torch.float64 or cn.numel() != Kp or cn.device != dev:
        raise ValueError(f"{name}: cn is float64 [{Kp}] on the CSR's device")
    if not all(0 <= int(e) <= lim["k_max"] for e in (k, kw, kc)):
        raise ValueError(f"{name}: scale exponents lie in 0 .. {lim['k_max']}")
    grp = _clu_rows(name, "group", group, n, dev)
    w = None if weights is None else torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
    if w is not None and w.numel() != n:
        raise ValueError(f"{name}: weights needs one entry per row")
    slot_of = hot_feat = None
    if sums and dev.type == "cuda":
        slot_of, hot_feat = hot if isinstance(hot, tuple) else hot_tables(indptr, idx, val, F, K, hot)
        if hot_feat is not None and hot_feat.numel() * 8 * K > lim["max_table_bytes"]:
            raise ValueError(f"{name}: the hot set exceeds the LDS table")
    out = torch.zeros((K * F if sums else 0) + 3 * K + 1, dtype=torch.int64, device=dev)
    assign = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
    dist = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    native.lib().km_group_step(indptr, idx, val, w, grp, W, G, CT.contiguous(), cn.contiguous(), m, int(k), int(kw),
                               int(kc), slot_of, hot_feat, out, bool(sums), assign, dist, int(chunk_rows), threads)
    blk = KmGroupBlock(out, F, K, bool(sums), assign, dist)
    if check and blk.flag:
        if bool(torch.any(grp >= G)):
            raise ValueError(f"{name}: a group lies outside 0 .. {G - 1}")
        live = grp >= 0                                   # a skipped row is not read, so it cannot be the bad one
        entries = torch.repeat_interleave(live, indptr[1:] - indptr[:-1])
        _raise_bad_input("km", idx[entries], val[entries], None, None if w is None else w[live], F)
    return blk


@dataclass
class SilBlock:
    """``[silq, wq, flag]`` of one ``sil_score`` on the CSR's device, and the per-row coefficients
    when they were asked for."""
    block: torch.Tensor
    s: Optional[torch.Tensor] = None

    @property
    def silq(self) -> int:
        return int(self.block[0])

    @property
    def wq(self) -> int:
        return int(self.block[1])

    @property
    def flag(self) -> int:
        return int(self.block[2])


def sil_score(vc, labels, K: int, MT: torch.Tensor, psi: torch.Tensor, nw: torch.Tensor, cnt: torch.Tensor,
              measure: str, ks: int, kw: int, weights=None, want_rows: bool = False, chunk_rows: int = 0,
              threads: int = 0, check: bool = True) -> SilBlock:
    """Spark's silhouette coefficient of every row, summed exactly. ``MT`` [F, Kp] fp64 are the
    cluster means, feature-major (cosine: the means of the rows divided by their norms), ``psi`` [Kp]
    (euclidean: the mean squared norm of a cluster's rows), ``nw`` [Kp] the weight sums (0 for an
    absent cluster) and ``cnt`` [Kp] int32 the row counts. A row with the label ``a``: the dots and
    the squared norm as in ``km_step`` (tiles of 8), ``D_c = (xn + psi_c) - 2 dot_c`` unclamped
    (cosine: ``1 - dot_c / sqrt(xn)``), ``own = D_a nw_a / (nw_a - w)``, ``nb`` the least ``D_c`` over the
    other present clusters (ascending, strict ``<``), ``s = 0`` for ``cnt_a == 1``, else ``1 - own / nb``,
    ``nb / own - 1`` or 0; ``silq += rint(w s 2^ks)``, ``wq += rint(w 2^kw)``. ``want_rows`` adds ``s`` per
    row. ``chunk_rows`` and ``threads`` change no bit. Raises ``ValueError`` before any launch for ``K``
    outside ``2 .. max_k``, an unknown measure or a shape mismatch, and with ``check`` after the pass
    for bad input: ``km_step``'s cases, a label outside ``0 .. K - 1`` or of an absent cluster, no other
    present cluster, ``nw_a - w`` not > 0 for a non-singleton, or a coefficient that is not finite."""
    name = "sil_score"
    lim = clu_limits()
    if not 2 <= int(K) <= lim["max_k"]:
        raise ValueError(f"{name}: 2 .. {lim['max_k']} clusters, got {K}")
    m = _clu_measure(name, measure)
    K, Kp = int(K), km_padded(K)
    indptr, idx, val = _csr(vc)
    dev, F, n = indptr.device, int(vc.size), indptr.numel() - 1
    if MT.dtype != torch.float64 or MT.dim() != 2 or tuple(MT.shape) != (F, Kp) or MT.device != dev:
        raise ValueError(f"{name}: MT is float64 [{F}, {Kp}] on the CSR's device")
    for what, t, dt in (("psi", psi, torch.float64), ("nw", nw, torch.float64), ("cnt", cnt, torch.int32)):
        if t.dtype != dt or t.numel() != Kp or t.device != dev:
            raise ValueError(f"{name}: {what} is {dt} [{Kp}] on the CSR's device")
    if not all(0 <= int(e) <= lim["k_max"] for e in (ks, kw)):
        raise ValueError(f"{name}: scale exponents lie in 0 .. {lim['k_max']}")
    lab = _clu_rows(name, "labels", labels, n, dev)
    w = None if weights is None else torch.as_tensor(weights).to(device=dev, dtype=torch.float64).contiguous()
    if w is not None and w.numel() != n:
        raise ValueError(f"{name}: weights needs one entry per row")
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    s = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
    native.lib().sil_score(indptr, idx, val, w, lab, K, MT.contiguous(), psi.contiguous(), nw.contiguous(),
                           cnt.contiguous(), m, int(ks), int(kw), out, s, int(chunk_rows), threads)
    blk = SilBlock(out, s)
    if check and blk.flag:
        if bool(torch.any((lab < 0) | (lab >= K))):
            raise ValueError(f"{name}: a label lies outside 0 .. {K - 1}")
        if bool(torch.any(nw[lab.to(torch.int64)] <= 0)):
            raise ValueError(f"{name}: a label names an absent cluster")
        if int((nw[:K] > 0).sum()) < 2:
            raise ValueError(f"{name}: the silhouette needs two clusters that are present")
        norms = sim_norms(indptr, val)
        if (w is not None and not bool(torch.all(torch.isfinite(w) & (w > 0)))) or not bool(torch.all(torch.isfinite(val))) \
                or (idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= F)) \
                or not bool(torch.all(torch.isfinite(norms * norms))) or (m == 1 and bool(torch.any(norms == 0))):
            _raise_bad_input("km", idx, val, None, w, F)
        raise ValueError(f"{name}: a coefficient is not finite, or a cluster's weight sum does not exceed a row's")
    return blk


def mlr_limits() -> dict:
    """Structural constants of the multinomial logistic-regression kernel: those of ``nb_limits`` it
    shares (``max_classes``, ``chunk_rows``, ``table_bytes``, ``max_table_bytes``, ``k_max``,
    ``sum_bits``, wave and workgroup size), the loss cap (``loss_cap = 2^loss_bits``) and the two
    halves of the flag word (``flag_clamped``, ``flag_bad_input``)."""
    return dict(native.lib().mlr_limits())


def mlr_scale_exponents(wmax: float, vmax: float, n_rows: int) -> tuple:
    """``(k, kl)`` of ``mlr_eval`` for weights up to ``wmax``, absolute values up to ``vmax`` and
    ``n_rows`` rows in all: ``k = min(k_max, sum_bits - n_rows.bit_length() - e)`` with
    ``max(wmax max(vmax, 1), 1) < 2^e`` (a residual is at most its row's weight) and
    ``kl = min(k_max, sum_bits - n_rows.bit_length() - e_w - loss_bits)`` with ``max(wmax, 1) < 2^e_w``
    (``frexp``). Raises ``ValueError`` when an exponent is negative."""
    lim = mlr_limits()
    wmax, vmax = float(wmax), float(vmax)
    if not (math.isfinite(wmax) and math.isfinite(vmax)) or wmax < 0 or vmax < 0:
        raise ValueError(f"multinomial logistic regression needs finite values and finite, non-negative weights "
                         f"(largest weight {wmax}, largest |value| {vmax})")
    room = int(lim["sum_bits"]) - int(n_rows).bit_length()
    k = min(int(lim["k_max"]), room - math.frexp(max(wmax * max(vmax, 1.0), 1.0))[1])
    kl = min(int(lim["k_max"]), room - math.frexp(max(wmax, 1.0))[1] - int(lim["loss_bits"]))
    if k < 0 or kl < 0:
        raise ValueError(f"weights up to {wmax:g} and values up to {vmax:g} over {n_rows} rows do not fit the exact "
                         f"{lim['sum_bits']}-bit sums of multinomial logistic regression")
    return k, kl


class _FlaggedBlock:
    """An int64 block whose last word is the flag word of ``csrc/fixedpoint.h``: the low half says
    that a row's loss was clamped, the high half names bad input."""
    block: torch.Tensor

    @property
    def flag(self) -> int:
        return int(self.block[-1])

    @property
    def clamped(self) -> bool:
        return bool(self.flag & 0xFFFFFFFF)

    @property
    def bad_input(self) -> bool:
        return bool(self.flag >> 32)


@dataclass
class MlrBlock(_FlaggedBlock):
    """The int64 block of one ``mlr_eval``: ``Gq`` [F, C] feature-major, ``gbq`` [C], ``lossq``, the
    two flags, and the per-row outputs when they were asked for."""
    block: torch.Tensor
    F: int
    C: int
    margin: Optional[torch.Tensor] = None
    R: Optional[torch.Tensor] = None
    loss_row: Optional[torch.Tensor] = None

    @property
    def Gq(self) -> torch.Tensor:
        return self.block[:self.F * self.C].view(self.F, self.C)

    @property
    def gbq(self) -> torch.Tensor:
        return self.block[self.F * self.C:self.F * self.C + self.C]

    @property
    def lossq(self) -> int:
        return int(self.block[-2])


def mlr_eval(indptr, idx, val, XS: torch.Tensor, b: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor],
             k: int, kl: int, hot_tables: tuple = (None, None), want_rows: bool = False, chunk_rows: int = 0,
             check_extents: bool = True, threads: int = 0) -> MlrBlock:
    """One evaluation of multinomial logistic regression on a CSR (``val`` fp32 or fp64) in one fused
    pass: margins bitwise ``score_csr(ClassLinearScorer(XS, b))``, the row terms of ``csrc/mlr.h``
    and the exact int64 sums ``Gq[f, c] = sum rint(x_if r_ic 2^k)``, ``gbq[c] = sum rint(r_ic 2^k)``,
    ``lossq = sum rint(w_i min(loss_i, 2048) 2^kl)``. ``XS`` is ``[F, C]`` fp64 feature-major.
    ``hot_tables`` is ``nb_hot_tables(...)`` of the features summed in LDS on the device (the host
    ignores it); like ``chunk_rows`` and ``threads`` it changes the speed only. The block stays on
    the CSR's device; nothing is read back here, the caller tests the flags."""
    dev = indptr.device
    F, C_ = int(XS.shape[0]), int(XS.shape[1])
    n = indptr.numel() - 1
    slot_of, hot_feat = hot_tables if dev.type == "cuda" else (None, None)
    out = torch.zeros(F * C_ + C_ + 2, dtype=torch.int64, device=dev)
    rows = [torch.empty(s, dtype=torch.float64, device=dev) if want_rows else None for s in ((n, C_), (n, C_), (n,))]
    native.lib().mlr_eval(indptr, idx, val, XS, b, y, w, int(k), int(kl), slot_of, hot_feat, out, rows[0], rows[1],
                          rows[2], int(chunk_rows), bool(check_extents), threads)
    return MlrBlock(out, F, C_, *rows)


def svc_limits() -> dict:
    """Structural constants of the linear SVC kernel: those of ``nb_limits`` it shares (``chunk_rows``,
    ``table_bytes``, ``max_table_bytes``, ``k_max``, ``sum_bits``, wave and workgroup size), the slots
    of the default and of the largest LDS table (``hot_slots``, ``max_hot_slots``), the loss cap
    (``loss_cap = 2^loss_bits``) and the two halves of the flag word (``flag_clamped``,
    ``flag_bad_input``)."""
    return dict(native.lib().svc_limits())


@dataclass
class SvcBlock(_FlaggedBlock):
    """The int64 block of one ``svc_eval``: ``Gq`` [F], ``gbq``, ``lossq``, ``nact``, the flag word,
    and the per-row outputs when they were asked for."""
    block: torch.Tensor
    F: int
    margin: Optional[torch.Tensor] = None
    r: Optional[torch.Tensor] = None
    loss_row: Optional[torch.Tensor] = None

    @property
    def Gq(self) -> torch.Tensor:
        return self.block[:self.F]

    @property
    def gbq(self) -> int:
        return int(self.block[self.F])

    @property
    def lossq(self) -> int:
        return int(self.block[self.F + 1])

    @property
    def nact(self) -> int:
        return int(self.block[self.F + 2])


def svc_eval(indptr, idx, val, xs: torch.Tensor, b: float, y: torch.Tensor, w: Optional[torch.Tensor],
             k: int, kl: int, hot_tables: tuple = (None, None), want_rows: bool = False, chunk_rows: int = 0,
             check_extents: bool = True, threads: int = 0) -> SvcBlock:
    """One evaluation of the linear SVC hinge objective on a CSR (``val`` fp32 or fp64) in one fused
    pass: margins bitwise ``spmv(X, xs) + b``, the row terms of ``csrc/svc.h`` and the exact int64
    sums ``Gq[f] = sum rint(x_if r_i 2^k)``, ``gbq = sum rint(r_i 2^k)``,
    ``lossq = sum rint(w_i min(loss_i, 2048) 2^kl)`` and ``nact``, the rows with a non-zero residual.
    ``(k, kl)`` come from ``mlr_scale_exponents``. The whole block is a pure function of the inputs
    and equal bit for bit on the host and the device: ``hot_tables`` (``nb_hot_tables(..., 1)`` of the
    features summed in LDS on the device; the host ignores it), ``chunk_rows`` and ``threads`` change
    the speed only. The block stays on the CSR's device; nothing is read back here, the caller tests
    the flags. Raises ``ValueError`` for arguments of the wrong shape, dtype or range."""
    lim = svc_limits()
    dev = indptr.device
    if indptr.dtype != torch.int64 or idx.dtype != torch.int32 or val.dtype not in (torch.float32, torch.float64):
        raise ValueError("svc_eval: the CSR is (indptr int64, idx int32, val float32 / float64)")
    if indptr.dim() != 1 or indptr.numel() < 1 or idx.numel() != val.numel():
        raise ValueError("svc_eval: indptr holds rows + 1 entries, idx / val one per entry")
    n = indptr.numel() - 1
    if xs.dim() != 1 or xs.numel() < 1 or xs.dtype != torch.float64:
        raise ValueError("svc_eval: xs is a float64 vector [F]")
    F = int(xs.numel())
    if y.dtype != torch.float64 or y.numel() != n:
        raise ValueError("svc_eval: labels are float64, one per row")
    if w is not None and (w.dtype != torch.float64 or w.numel() != n):
        raise ValueError("svc_eval: weights are float64, one per row")
    if any(t.device != dev for t in (idx, val, xs, y) + (() if w is None else (w,))):
        raise ValueError("svc_eval: every tensor lives on the CSR's device")
    if not (0 <= int(k) <= lim["k_max"] and 0 <= int(kl) <= lim["k_max"]):
        raise ValueError(f"svc_eval: scale exponents lie in 0 .. {lim['k_max']}")
    if not 0 <= int(chunk_rows) <= (1 << 20):
        raise ValueError("svc_eval: chunk_rows out of range")
    slot_of, hot_feat = hot_tables if dev.type == "cuda" else (None, None)
    if (slot_of is None) != (hot_feat is None):
        raise ValueError("svc_eval: slot_of and hot_feat come together")
    if hot_feat is not None and (hot_feat.numel() * 8 > lim["max_table_bytes"] or slot_of.numel() != F):
        raise ValueError("svc_eval: the hot set exceeds the LDS table or does not cover the feature space")
    out = torch.zeros(F + 4, dtype=torch.int64, device=dev)
    rows = [torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None for _ in range(3)]
    native.lib().svc_eval(indptr.contiguous(), idx.contiguous(), val.contiguous(), xs.contiguous(), float(b),
                          y.contiguous(), None if w is None else w.contiguous(), int(k), int(kl), slot_of, hot_feat,
                          out, rows[0], rows[1], rows[2], int(chunk_rows), bool(check_extents), threads)
    return SvcBlock(out, F, *rows)


def softprob_limits() -> dict:
    """Structural constants of the multi-class boosting kernels: ``max_classes``, workgroup size
    (``block``), ``wave`` and the hessian floor (``min_hess``)."""
    return dict(native.lib().softprob_limits())


def _check_classes(C_: int) -> None:
    lim = int(softprob_limits()["max_classes"])
    if not 2 <= C_ <= lim:
        raise ValueError(f"the class count must lie in 2 .. {lim}, got {C_}")


def softprob_grad(margin: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor], g: torch.Tensor,
                  h: torch.Tensor, threads: int = 0) -> None:
    """The gradient planes of ``multi:softprob`` in one launch (``csrc/softprob.h``): ``margin`` is
    ``[C, N]`` fp64, ``y`` ``[N]`` fp32 labels (integers ``0 .. C - 1``; only compared, never an
    index), ``w`` ``[N]`` fp32 or ``None`` (1.0); ``g`` and ``h`` are ``[C, N]`` fp32 planes whose rows
    are contiguous (a plane may be a view of a wider buffer) and of which exactly ``[c, :N]`` is written.
    Everything is checked here, before the launch."""
    if margin.dim() != 2:
        raise ValueError("margin is [C, N]")
    C_, n = int(margin.shape[0]), int(margin.shape[1])
    _check_classes(C_)
    for name, t, dt in (("margin", margin, torch.float64), ("g", g, torch.float32), ("h", h, torch.float32)):
        if t.dtype != dt or t.device != margin.device:
            raise ValueError(f"{name} must be {dt} on the margins' device")
        if t.dim() != 2 or tuple(t.shape) != (C_, n):
            raise ValueError(f"{name} must be [C, N] = [{C_}, {n}], got {tuple(t.shape)}")
        if (n > 1 and t.stride(1) != 1) or t.stride(0) < n:
            raise ValueError(f"{name}: the rows of a plane must be contiguous and the planes disjoint")
    for name, t in (("y", y), ("w", w)):
        if t is None and name == "w":
            continue
        if t.dtype != torch.float32 or t.device != margin.device or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 vector on the margins' device")
        if t.numel() != n:
            raise ValueError(f"{name} needs one entry per row ({n}), got {t.numel()}")
    native.lib().softprob_grad(margin, y, w, g, h, threads)


def score_class_trees(vc, arrays, threads: int = 0) -> torch.Tensor:
    """Raw class scores ``[N, C]`` fp64 of a class-grouped tree list (``ClassTreeArrays``):
    ``raw[r, c]`` is the sum of the leaf values of the trees of class ``c`` in the order of
    ``csrc/softprob.h`` (64 lane-strided partials, the xor butterfly); a class without a tree gives
    ``+0.0``. Everything is checked here, before the launch."""
    from .text import ClassTreeArrays

    if not isinstance(arrays, ClassTreeArrays):
        raise TypeError(f"score_class_trees takes ClassTreeArrays, got {type(arrays)}")
    C_ = int(arrays.num_classes)
    _check_classes(C_)
    tc = arrays.tree_class
    if tc.size != arrays.roots.size:
        raise ValueError("tree_class needs one entry per tree")
    if tc.size and (int(tc.min()) < 0 or int(tc.max()) >= C_):
        raise ValueError(f"a tree's class id lies outside 0 .. {C_ - 1}")
    if arrays.max_feature() >= vc.size:
        raise ValueError("tree references a feature beyond the feature space")
    indptr, idx, val = _csr(vc)
    dev = indptr.device
    n = indptr.numel() - 1
    out = torch.empty((n, C_), dtype=torch.float64, device=dev)
    t = arrays.tensors(dev)
    native.lib().score_class_trees(indptr, idx, val, t[:6], t[6], C_, arrays.cmp_less, out, threads)
    return out


def sim_limits() -> dict:
    """Structural constants of the retrieval kernels: largest ``k``, distinct terms of a query held
    in LDS, corpus rows per workgroup chunk, queries per pass over a chunk, wave and workgroup size."""
    return dict(native.lib().sim_limits())


@dataclass
class SimIndex:
    """A CSR corpus prepared for ``topk_cosine``: ``norms[r] = sqrt(sum val^2)`` in spmv's order."""
    indptr: torch.Tensor
    idx: torch.Tensor
    val: torch.Tensor
    norms: torch.Tensor
    size: int

    @property
    def rows(self) -> int:
        return int(self.indptr.numel() - 1)


def sim_norms(indptr: torch.Tensor, val: torch.Tensor, threads: int = 0) -> torch.Tensor:
    norms = torch.empty(indptr.numel() - 1, dtype=torch.float64, device=indptr.device)
    native.lib().sim_norms(indptr, val, norms, threads)
    return norms


def sim_index(vc, threads: int = 0) -> SimIndex:
    """Index of a ``VectorColumn`` whose rows hold ascending, distinct feature ids (what the
    featurizer writes)."""
    indptr, idx, val = _csr(vc)
    if indptr.numel() < 1 or int(indptr[0]) != 0 or int(indptr[-1]) != idx.numel():
        raise ValueError("indptr does not span the CSR's entries")
    return SimIndex(indptr, idx, val, sim_norms(indptr, val, threads), int(vc.size))


def topk_cosine(index: SimIndex, queries_vc, k: int, threads: int = 0, chunk_rows: int = 0,
                queries_per_pass: int = 0):
    """Exact top-``k`` cosine neighbours of every row of ``queries_vc`` among the index's rows:
    ``(rows int64 [Q, min(k, N)], sims float64 [Q, min(k, N)])`` by descending similarity, ties by
    ascending row. ``dot(r, q)`` is ``spmv(corpus, dense(q))[r]`` bit for bit and
    ``sim = dot / max(norm[r] * |q|, 1e-12)``, so the result is a pure function of (corpus, queries,
    k): ``chunk_rows`` and ``queries_per_pass`` (0 = default) only change how the work is split. A
    query with more than ``query_cap`` distinct terms takes the dense-query path (``spmv``, the same
    division, a stable descending argsort): the same contract and the same bits."""
    lim = sim_limits()
    k = int(k)
    if not 1 <= k <= lim["k_max"]:
        raise ValueError(f"k must lie in 1 .. {lim['k_max']}")
    if queries_vc.size != index.size:
        raise ValueError("queries and corpus live in different feature spaces")
    q_indptr, q_idx, q_val = _csr(queries_vc)
    dev = index.indptr.device
    if q_indptr.device != dev:
        raise ValueError("queries and corpus live on different devices")
    q_val = q_val.to(torch.float64)
    Q, N = int(q_indptr.numel() - 1), index.rows
    kk = min(k, N)
    rows = torch.empty((Q, kk), dtype=torch.int64, device=dev)
    sims = torch.empty((Q, kk), dtype=torch.float64, device=dev)
    if Q == 0 or N == 0:
        return rows, sims
    C = native.lib()
    qp = q_indptr.cpu()
    long_q = torch.nonzero(qp[1:] - qp[:-1] > lim["query_cap"]).flatten().tolist()
    if not long_q:
        C.sim_topk(index.indptr, index.idx, index.val, index.norms, q_indptr, q_idx, q_val, k, rows, sims,
                   chunk_rows, queries_per_pass, threads)
        return rows, sims
    is_long = set(long_q)
    short = [q for q in range(Q) if q not in is_long]
    if short:
        sel = torch.tensor(short, dtype=torch.int64)
        lens = (qp[1:] - qp[:-1])[sel]
        sp = torch.zeros(len(short) + 1, dtype=torch.int64)
        torch.cumsum(lens, 0, out=sp[1:])
        take = torch.cat([torch.arange(int(qp[q]), int(qp[q + 1])) for q in short]).to(dev)
        r_s = torch.empty((len(short), kk), dtype=torch.int64, device=dev)
        s_s = torch.empty((len(short), kk), dtype=torch.float64, device=dev)
        C.sim_topk(index.indptr, index.idx, index.val, index.norms, sp.to(dev), q_idx[take].contiguous(),
                   q_val[take].contiguous(), k, r_s, s_s, chunk_rows, queries_per_pass, threads)
        rows[sel.to(dev)] = r_s
        sims[sel.to(dev)] = s_s
    q_norms = sim_norms(q_indptr, q_val, threads)
    for q in long_q:
        a, b = int(qp[q]), int(qp[q + 1])
        x = torch.zeros(index.size, dtype=torch.float64, device=dev)
        x[q_idx[a:b].to(torch.int64)] = q_val[a:b]
        dot = spmv(index.indptr, index.idx, index.val, x, threads)
        s = dot / torch.clamp(index.norms * q_norms[q], min=1e-12)
        top = torch.argsort(s, descending=True, stable=True)[:kk]
        rows[q], sims[q] = top, s[top]
    return rows, sims


def term_presence_by_label(vc, term_ids, labels, num_classes: int = 2) -> torch.Tensor:
    """K-19: documents containing each of ``term_ids`` per label, in one pass over the CSR
    (replaces the reference's one Spark job per word, fraud_detection_spark.py:256-269).
    Returns ``counts[len(term_ids), num_classes]`` (int64)."""
    indptr, idx, val = vc.csr()
    dev = indptr.device
    ids = torch.as_tensor(term_ids, dtype=torch.int64, device=dev)
    lab = torch.as_tensor(labels, device=dev).to(torch.int64)
    slot = torch.full((vc.size,), -1, dtype=torch.int64, device=dev)
    slot[ids] = torch.arange(ids.numel(), device=dev)
    row = torch.repeat_interleave(torch.arange(indptr.numel() - 1, device=dev), indptr[1:] - indptr[:-1],
                                  output_size=int(idx.numel()))
    s = slot[idx.to(torch.int64)]
    keep = (s >= 0) & (val != 0)
    key = s[keep] * num_classes + lab[row[keep]]
    return torch.bincount(key, minlength=ids.numel() * num_classes).view(ids.numel(), num_classes)


def doc_freq(idx: torch.Tensor, val: torch.Tensor, size: int) -> torch.Tensor:
    if idx.is_cuda:
        df = torch.zeros(size, dtype=torch.int64, device=idx.device)
        native.lib().doc_freq(idx.to(torch.int32).contiguous(), val.contiguous(), df)
        return df
    return torch.bincount(idx[val != 0].to(torch.int64), minlength=size)


@dataclass
class FeatureOrder:
    """Column-major (CSC) view of a count CSR: ``csc_row`` / ``csc_cnt`` (min(count, 255)) are
    views with >= 16 readable padding entries behind them, ``colptr`` [F+1], ``df`` document
    frequencies and ``maxc`` per-feature maximum count."""
    csc_row: torch.Tensor
    csc_cnt: torch.Tensor
    colptr: torch.Tensor
    df: torch.Tensor
    maxc: torch.Tensor
    # features whose entries were dropped from csc_row / csc_cnt (drop_features; df keeps them)
    dropped: Optional[torch.Tensor] = None

    def drop_features(self, drop: torch.Tensor) -> None:
        """Remove the entries of the features flagged in ``drop`` [F] (bool) IN PLACE: the kept
        columns slide left over the dropped ones, in order, so no second CSC is allocated (the
        trainers drop features whose values are all zero, e.g. IDF 0 for terms in every
        document, whose columns hold one entry per row: copying the rest of the CSC instead
        cost 5 B per entry of transient HBM). Every move copies ``chunk <= shift`` entries, so
        source and destination of one copy never overlap; copies run in stream order."""
        colptr = self.colptr.cpu().numpy()
        dmask = drop.cpu().numpy().astype(bool)
        lens = np.diff(colptr)
        dmask &= lens > 0
        if not dmask.any():
            return
        nnz = int(colptr[-1])
        # maximal runs of kept columns -> (src start, src end)
        edges = np.flatnonzero(np.diff(np.concatenate([[1], dmask.astype(np.int8), [1]])))
        dst = 0
        for a, b in zip(edges[0::2], edges[1::2]):          # kept features [a, b)
            s0, s1 = int(colptr[a]), int(colptr[b])
            n = s1 - s0
            if n and s0 != dst:
                shift = s0 - dst
                for off in range(0, n, shift):
                    c = min(shift, n - off)
                    self.csc_row[dst + off:dst + off + c].copy_(self.csc_row[s0 + off:s0 + off + c])
                    self.csc_cnt[dst + off:dst + off + c].copy_(self.csc_cnt[s0 + off:s0 + off + c])
            dst += n
        new_lens = np.where(dmask, 0, lens)
        newptr = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.int64)
        assert int(newptr[-1]) == dst <= nnz
        self.colptr.copy_(torch.from_numpy(newptr))
        self.csc_row, self.csc_cnt = self.csc_row[:dst], self.csc_cnt[:dst]
        d = torch.from_numpy(dmask).to(self.maxc.device)
        self.dropped = d if self.dropped is None else (self.dropped | d)


# entries radix-sorted at once by feature_order: the device sort needs 24 B of temporaries per
# entry, so a 1.25B-entry shard sorts in row blocks of this size (each block's columns are copied
# into place; rows stay in row order within every column, exactly the one-shot CSC)
FO_BLOCK_ENTRIES = int(os.environ.get("FDX_FO_BLOCK_ENTRIES", 1 << 28))


def _feature_order_one(indptr, idx, counts, num_features: int, row_buf, cnt_buf) -> tuple:
    dev = idx.device
    nnz = int(idx.numel())
    colptr = torch.empty(num_features + 1, dtype=torch.int64, device=dev)
    df = torch.empty(num_features, dtype=torch.int64, device=dev)
    maxc = torch.empty(num_features, dtype=torch.int32, device=dev)
    native.lib().feature_order(indptr.contiguous(), idx.to(torch.int32).contiguous(), counts.contiguous(),
                               int(num_features), row_buf[:nnz], cnt_buf[:nnz], colptr, df, maxc)
    return colptr, df, maxc


def feature_order(indptr: torch.Tensor, idx: torch.Tensor, counts: torch.Tensor, num_features: int,
                  block_entries: Optional[int] = None) -> FeatureOrder:
    """CSR (rows, sorted unique feature ids per row, term counts) -> CSC by feature with a native
    radix sort; docFreq and the per-feature max count are segmented reductions (no atomics).
    Integer counts are sorted as int32 (no float copy). Above ``block_entries`` entries the rows
    are sorted in blocks, so the sort's temporaries stay bounded (HBM sizing)."""
    dev = idx.device
    nnz = int(idx.numel())
    if counts.dtype not in (torch.float32, torch.float64, torch.int32):
        counts = counts.to(torch.float32 if counts.is_floating_point() else torch.int32)
    pad = 16
    row_buf = torch.zeros(nnz + pad, dtype=torch.int32, device=dev)
    cnt_buf = torch.zeros(nnz + pad, dtype=torch.uint8, device=dev)
    block = int(block_entries or FO_BLOCK_ENTRIES)
    if nnz <= block:
        colptr, df, maxc = _feature_order_one(indptr, idx, counts, num_features, row_buf, cnt_buf)
        return FeatureOrder(row_buf[:nnz], cnt_buf[:nnz], colptr, df, maxc)
    N = int(indptr.numel() - 1)
    # row blocks of <= ~block entries (a single row larger than a block is its own block)
    targets = torch.arange(block, nnz, block, dtype=torch.int64, device=dev)
    cuts = torch.searchsorted(indptr, targets, right=True).clamp(1, N) - 1
    rcuts = sorted(set([0, N] + [int(c) for c in cuts.cpu().tolist() if 0 < int(c) < N]))
    C = native.lib()
    # pass 1: per-block column sizes (one bincount per block) -> every block's column offsets
    lens = []
    for r0, r1 in zip(rcuts[:-1], rcuts[1:]):
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        lens.append(torch.bincount(idx[e0:e1].to(torch.int64), minlength=num_features))
    tot = torch.stack(lens).sum(0)
    colptr = torch.zeros(num_features + 1, dtype=torch.int64, device=dev)
    torch.cumsum(tot, 0, out=colptr[1:])
    df = torch.zeros(num_features, dtype=torch.int64, device=dev)
    maxc = torch.zeros(num_features, dtype=torch.int32, device=dev)
    before = torch.zeros(num_features, dtype=torch.int64, device=dev)
    # pass 2: sort each block, add its first row, copy its columns into place (one block's
    # temporaries alive at a time; IncrementalFeatureOrder keeps every block until the end)
    for (r0, r1), ln in zip(zip(rcuts[:-1], rcuts[1:]), lens):
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        n = e1 - e0
        brow = torch.zeros(n + pad, dtype=torch.int32, device=dev)
        bcnt = torch.zeros(n + pad, dtype=torch.uint8, device=dev)
        bcol, bdf, bmax = _feature_order_one(indptr[r0:r1 + 1] - e0, idx[e0:e1], counts[e0:e1], num_features, brow,
                                             bcnt)
        brow[:n] += r0
        df += bdf                        # entries with a positive count, as in the one-shot order
        torch.maximum(maxc, bmax, out=maxc)
        C.copy_segments(brow[:n], bcnt[:n], bcol[:-1].contiguous(), (colptr[:-1] + before).contiguous(), ln,
                        row_buf[:nnz], cnt_buf[:nnz], None)
        before += ln
        del brow, bcnt, bcol
    return FeatureOrder(row_buf[:nnz], cnt_buf[:nnz], colptr, df, maxc)


class IncrementalFeatureOrder:
    """feature_order built one row block at a time, as the blocks arrive (e.g. each featurized
    chunk while the next chunk's raw text is still crossing PCIe): every block is sorted by
    feature on its own (``add``), and ``finish`` copies each block's columns into place behind the
    earlier blocks' entries of the same column. Rows stay ascending within every column, so the
    result equals the one-shot CSC of the concatenated CSR. Holds every block's sorted (row, count)
    pairs until ``finish`` (5 B per entry on top of the CSR, then the same again for the output)."""

    PAD = 16

    def __init__(self, num_features: int, device):
        self.F, self.dev = int(num_features), torch.device(device)
        self.blocks: list = []               # (block colptr, rows (global), counts u8, n entries)
        self.maxc = torch.zeros(self.F, dtype=torch.int32, device=self.dev)
        self.df = torch.zeros(self.F, dtype=torch.int64, device=self.dev)    # entries with a positive count
        self.nnz = 0

    def add(self, indptr: torch.Tensor, idx: torch.Tensor, counts: torch.Tensor, first_row: int) -> None:
        """Sort one block: ``indptr`` local to the block (starts at 0), rows ``first_row + i``."""
        if counts.dtype not in (torch.float32, torch.float64, torch.int32):
            counts = counts.to(torch.float32 if counts.is_floating_point() else torch.int32)
        n = int(idx.numel())
        brow = torch.zeros(n + self.PAD, dtype=torch.int32, device=self.dev)
        bcnt = torch.zeros(n + self.PAD, dtype=torch.uint8, device=self.dev)
        bcol, bdf, bmax = _feature_order_one(indptr, idx, counts, self.F, brow, bcnt)
        if first_row:
            brow[:n] += int(first_row)
        self.df += bdf
        torch.maximum(self.maxc, bmax, out=self.maxc)
        self.blocks.append((bcol, brow, bcnt, n))
        self.nnz += n

    def finish(self) -> FeatureOrder:
        nnz, dev = self.nnz, self.dev
        lens = [bcol[1:] - bcol[:-1] for bcol, _, _, _ in self.blocks]
        tot = torch.stack(lens).sum(0) if lens else torch.zeros(self.F, dtype=torch.int64, device=dev)
        colptr = torch.zeros(self.F + 1, dtype=torch.int64, device=dev)
        torch.cumsum(tot, 0, out=colptr[1:])
        if len(self.blocks) == 1:               # one block: its sort is the CSC
            _, brow, bcnt, n = self.blocks.pop()
            return FeatureOrder(brow[:n], bcnt[:n], colptr, self.df, self.maxc)
        row_buf = torch.zeros(nnz + self.PAD, dtype=torch.int32, device=dev)
        cnt_buf = torch.zeros(nnz + self.PAD, dtype=torch.uint8, device=dev)
        before = torch.zeros(self.F, dtype=torch.int64, device=dev)
        C = native.lib()
        for (bcol, brow, bcnt, n), ln in zip(self.blocks, lens):
            C.copy_segments(brow[:n], bcnt[:n], bcol[:-1].contiguous(), (colptr[:-1] + before).contiguous(), ln,
                            row_buf[:nnz], cnt_buf[:nnz], None)
            before += ln
        self.blocks = []
        return FeatureOrder(row_buf[:nnz], cnt_buf[:nnz], colptr, self.df, self.maxc)
