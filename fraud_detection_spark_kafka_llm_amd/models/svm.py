"""Linear support vector classification (Spark's ``LinearSVC``): hinge loss with an L2 penalty,
minimised by the L-BFGS loop of ``models/lr.py`` on the subgradient (Spark runs OWL-QN with no L1
part, which is the same method). One evaluation is one fused ``ops.sparse.svc_eval`` pass whose
reduced quantities are exact int64 sums of exactly rounded fp64 terms, so the loss and the gradient
of a parameter vector are the same bits on the host, on the device and for every world size."""
from __future__ import annotations

import math

import torch

from ..ops.sparse import _csr as sparse_csr
from ..ops.sparse import mlr_scale_exponents, svc_eval, svc_limits
from ._linear_common import (_raise_bad_input, coerce_rows, hot_tables, reduce_statistics, signed_extremes,
                             weight_sum_and_scale)
from .lr import _lbfgs

# counters of the last fit (evaluations, iterations, the scale exponents and the share of rows with a
# non-zero residual in the last evaluation): read by the profile note and the micro-benchmark only
SVC_STATS = {"evaluations": 0, "iterations": 0, "k": 0, "kl": 0, "active_share": 0.0}


def train_linear_svc(features, labels, weights=None, max_iter: int = 100, tol: float = 1e-6,
                     reg_param: float = 0.0, fit_intercept: bool = True, standardization: bool = True, device=None,
                     history_size: int = 10, hot=None, chunk_rows: int = 0, threads: int = 0):
    """Spark's ``LinearSVC``: minimises ``(1/W) sum_i w_i max(0, 1 - (2 y_i - 1) m_i) + regParam/2 |beta|^2``
    with ``m_i = b + sum_j x_ij s_j beta_j`` (``s`` = 1 / std of a feature with ``standardization``, 1
    without; the intercept is not penalised) from ``beta = 0``, ``b = 0`` by the L-BFGS loop of the
    binomial route. One evaluation is one fused ``ops.sparse.svc_eval`` pass; under data parallelism
    it all-reduces that one int64 block. Labels are 0 or 1. Returns ``(coefficients [F] = s beta,
    intercept, objective history)``. ``hot`` (feature ids summed in LDS on the device, ``None`` =
    ``nb_hot_set``), ``chunk_rows`` and ``threads`` change the speed only."""
    if reg_param < 0:
        raise ValueError(f"reg_param must be >= 0, got {reg_param}")
    dev, vc, y, w, n = coerce_rows(features, labels, weights, device)
    indptr, idx, val = sparse_csr(vc)
    F = int(vc.size)
    # the sixth statistic: rows whose label is neither 0 nor 1
    odd_rows = ((y != 0) & (y != 1)).sum().to(torch.float64)
    (ymax, ymin_neg, wmax, wmin_neg, vmax, odd), n_global = reduce_statistics(
        signed_extremes(y, w, val, n) + [odd_rows], n, dev)
    if not (math.isfinite(ymax) and math.isfinite(ymin_neg)) or odd != 0:
        raise ValueError("LinearSVC labels must be 0 or 1")
    if not (math.isfinite(wmax) and math.isfinite(wmin_neg)) or wmin_neg > 0:
        raise ValueError("LinearSVC weights must be finite and >= 0")
    if not math.isfinite(vmax):
        raise ValueError("LinearSVC requires finite feature values")
    k, kl = mlr_scale_exponents(wmax, vmax, n_global)
    coll, _, wsum, scale = weight_sum_and_scale(indptr, idx, val, F, w, n, standardization, "LinearSVC")
    tables = hot_tables(indptr, idx, val, F, 1, hot)
    inv_k = math.ldexp(1.0, -k)
    lim = svc_limits()
    stats_ = SVC_STATS
    stats_.update(evaluations=0, iterations=0, k=k, kl=kl, active_share=0.0)

    def fg(theta: torch.Tensor):
        beta = theta[:F]
        # one copy per evaluation: the intercept travels as a kernel argument
        b = float(theta[F]) if fit_intercept else 0.0
        res = svc_eval(indptr, idx, val, scale * beta, b, y, w, k, kl, tables, chunk_rows=chunk_rows,
                       check_extents=stats_["evaluations"] == 0, threads=threads)
        block = coll.sum(res.block)
        gbq, lossq, nact, flag = (int(v) for v in block[F:].cpu())
        if flag >> 32:
            _raise_bad_input("svc", idx, val, y, w, F)
        first = stats_["evaluations"] == 0
        stats_["evaluations"] += 1
        stats_["active_share"] = nact / max(n_global, 1)
        g = torch.empty_like(theta)
        g[:F] = scale * (block[:F].to(torch.float64) * inv_k) / wsum + reg_param * beta
        g[F] = math.ldexp(float(gbq), -k) / wsum if fit_intercept else 0.0
        if flag & 0xFFFFFFFF:       # a clamped row loss: the trial is rejected like an infinite objective
            if first:
                raise ValueError("LinearSVC: a row's loss at the starting point is not below "
                                 f"{int(lim['loss_cap'])} (margins out of range)")
            return math.inf, g
        loss = math.ldexp(float(lossq), -kl) / wsum + 0.5 * reg_param * float(torch.dot(beta, beta))
        return loss, g

    theta = torch.zeros(F + 1, dtype=torch.float64, device=dev)
    theta, history = _lbfgs(fg, theta, max_iter, tol, history_size)
    stats_["iterations"] = len(history) - 1
    coef = (scale * theta[:F]).cpu().numpy()
    intercept = float(theta[F]) if fit_intercept else 0.0
    return coef, intercept, history
