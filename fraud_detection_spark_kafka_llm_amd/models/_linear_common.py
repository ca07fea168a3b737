"""What the linear trainers (``lr.py``, ``svm.py``, ``nb.py``) share in front of their first pass:
input coercion, the stacked statistics that fix the scale exponents (one MAX and one SUM all-reduce),
the weight sum and the feature scale. Re-exported from ``ops.sparse``, where ``nb_sums`` needs them
too: the default-or-given hot tables of the device pass (``hot_tables``) and the ladder that names
bad input (``_raise_bad_input``). Each trainer keeps its own label rule, its ``fg`` and its
finalisation."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..ml.linalg import VectorColumn
from ..ops.sparse import _raise_bad_input, hot_tables, spmv  # noqa: F401
from ..parallel import dist as D
from ..parallel.dist import Collectives
from ..utils.config import default_device


def transpose_csr(indptr: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, num_cols: int) -> tuple:
    """CSR of X^T: entries stably sorted by column, so each column keeps its rows ascending."""
    n = indptr.numel() - 1
    counts = indptr[1:] - indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=idx.device), counts,
                                   output_size=int(idx.numel()))
    order = torch.sort(idx.to(torch.int64), stable=True).indices
    t_indptr = torch.zeros(num_cols + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(torch.bincount(idx.to(torch.int64), minlength=num_cols), 0, out=t_indptr[1:])
    return t_indptr, rows[order].contiguous(), val[order].contiguous()


def _feature_scale(xt, t_val, w, wsum, coll, F: int, standardization: bool) -> torch.Tensor:
    """``1 / std`` of every feature (sample std over all ranks, constant features 0) with
    ``standardization``, ones without; ``xt(v, vals)`` is the fixed-order ``X^T v``."""
    if standardization:
        s1 = coll.sum(xt(w))
        s2 = coll.sum(xt(w, t_val * t_val))
        mean = s1 / wsum
        var = (s2 - wsum * mean * mean) / max(wsum - 1.0, 1.0)
        std = torch.sqrt(torch.clamp(var, min=0.0))
        scale = torch.where(std > 0, 1.0 / torch.where(std > 0, std, torch.ones_like(std)), torch.zeros_like(std))
    else:
        scale = torch.ones(F, dtype=torch.float64, device=w.device)
    return scale


def coerce_rows(features, labels, weights, device):
    """``(dev, vc, y, w, n)``: the column on the device, labels and weights (``None`` = all 1) as
    contiguous float64 tensors there, ``n`` rows. Raises ``ValueError`` unless there is one label and
    one weight per row."""
    dev = torch.device(device) if device is not None else default_device()
    vc = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    vc = vc.to(dev)
    n = len(vc)
    y = torch.as_tensor(labels if isinstance(labels, (torch.Tensor, np.ndarray)) else
                        np.asarray([float(v) for v in labels])).to(device=dev, dtype=torch.float64).contiguous()
    w = None if weights is None else torch.as_tensor(
        weights if isinstance(weights, (torch.Tensor, np.ndarray)) else np.asarray(weights, dtype=np.float64)
    ).to(device=dev, dtype=torch.float64).contiguous()
    if y.numel() != n or (w is not None and w.numel() != n):
        raise ValueError("labels and weights need one entry per row")
    return dev, vc, y, w, n


def signed_extremes(y, w, val, n: int) -> list:
    """(largest label, - smallest label, largest weight, - smallest weight, largest |value|) as 0-d
    float64 tensors; no weights count as 1, no rows or entries as 0."""
    zero, one = y.new_zeros(()), y.new_ones(())
    return [y.max() if n else zero, -y.min() if n else zero,
            w.max() if w is not None and n else one, -w.min() if w is not None and n else -one,
            val.abs().max().to(torch.float64) if val.numel() else zero]


def reduce_statistics(stats: list, n: int, dev) -> tuple:
    """``(statistics as floats, rows over all ranks)``: the 0-d tensors ``stats`` travel as one small
    copy, MAX over the ranks (a NaN survives every maximum), the row count as one SUM."""
    stats = torch.stack(stats)
    rows = torch.tensor([n], dtype=torch.int64, device=dev)
    if D.is_dist():
        stats = D.all_reduce_max(stats)
        rows = D.all_reduce_sum(rows)
    return [float(v) for v in stats.cpu()], int(rows[0])


def weight_sum_and_scale(indptr, idx, val, F: int, w: Optional[torch.Tensor], n: int, standardization: bool,
                         family: str) -> tuple:
    """``(coll, w_rows, wsum, scale)``: the collectives of the fit, the weights as a tensor, their
    sum over all ranks (``ValueError`` naming ``family`` unless it is positive) and the feature scale
    (``_feature_scale``; the transposed CSR it needs lives only in here)."""
    coll = Collectives()
    w_rows = torch.ones(n, dtype=torch.float64, device=indptr.device) if w is None else w
    wsum = float(coll.sum(w_rows.sum().reshape(1))[0])
    if not wsum > 0:
        raise ValueError(f"{family} needs a positive weight sum")
    if not standardization:
        return coll, w_rows, wsum, _feature_scale(None, None, w_rows, wsum, coll, F, False)
    t_indptr, t_idx, t_val = transpose_csr(indptr, idx, val.to(torch.float64), F)

    def xt(v: torch.Tensor, vals: Optional[torch.Tensor] = None) -> torch.Tensor:
        return spmv(t_indptr, t_idx, t_val if vals is None else vals, v)

    return coll, w_rows, wsum, _feature_scale(xt, t_val, w_rows, wsum, coll, F, True)

