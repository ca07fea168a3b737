"""Binary logistic regression trainer (X-08): L-BFGS on the (weighted) mean log-loss.

Mirrors Spark ``LogisticRegression`` (binomial) as far as its semantics are defined: features are
standardized by their sample standard deviation when ``standardization=true`` (constant features
get coefficient 0), the L2 penalty ``regParam/2 * ||beta||^2`` acts on the standardized
coefficients, the intercept is unpenalised, L-BFGS keeps 10 correction pairs and stops after
``maxIter`` iterations or when the relative loss improvement falls below ``tol``. Spark's exact
iterate sequence (Breeze line search, virtual centering) is not reproduced, so coefficients match
Spark only at the optimum ("parity unpinned" for separable data, where both diverge until maxIter).

Hot ops run natively: margins ``X @ (s * beta)`` via ``csrc/sparse_kernels.hip::spmv_kernel`` and
the gradient ``X^T r`` as the same row-wise SpMV over ``X^T`` (built once per fit by a stable sort
of the entries by feature): every output is one fixed-order lane-strided dot product, no atomics,
so repeated fits are bitwise identical on the GPU. Under data parallelism each rank holds a row
shard and the gradient / loss / weight sums are all-reduced once per function evaluation (PAR-04).

With ``regParam > 0`` and ``elasticNetParam > 0`` the objective gains the L1 term
``regParam * (alpha * ||beta||_1 + (1 - alpha)/2 * ||beta||^2)`` and the trainer is OWL-QN (``_train_owlqn``)
on the fused kernels of ``csrc/lr_kernels.hip``: coefficients that leave their orthant are exactly 0.0.
Every other parameter pair runs the L-BFGS body below unchanged.

``train_multinomial_logistic_regression`` fits ``C`` coefficient rows (softmax, L2 penalty) with the same
L-BFGS loop; one evaluation is the fused ``ops.sparse.mlr_eval`` pass (``csrc/mlr_kernels.hip``), whose
gradient and loss are exact int64 fixed-point sums, so no transposed matrix is built.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ..ml.linalg import VectorColumn
from ..ops import native
from ..ops.sparse import _csr as sparse_csr
from ..ops.sparse import lr_forward, lr_owlqn_step, lr_pseudo_grad, mlr_eval, mlr_limits, mlr_scale_exponents, spmv
from ..parallel import dist as D
from ..parallel.dist import Collectives
from ..utils.config import default_device
from ._linear_common import (_feature_scale, _raise_bad_input, coerce_rows, hot_tables, reduce_statistics,
                             signed_extremes, transpose_csr, weight_sum_and_scale)


def _lbfgs(fg, theta: torch.Tensor, max_iter: int, tol: float, history_size: int):
    """L-BFGS on ``fg(theta) -> (loss, gradient)`` from ``theta``: ``history_size`` correction pairs,
    Armijo halving, stops after ``max_iter`` iterations, when the relative improvement falls below
    ``tol`` or the gradient norm below 1e-9. Returns ``(theta, objective history)``."""
    loss, g = fg(theta)
    history = [loss]
    S, Y = [], []
    for it in range(max_iter):
        # two-loop recursion
        q = g.clone()
        alphas = []
        for s, yv in reversed(list(zip(S, Y))):
            rho = 1.0 / float(torch.dot(yv, s))
            a = rho * float(torch.dot(s, q))
            alphas.append((a, rho, s, yv))
            q -= a * yv
        if S:
            gamma = float(torch.dot(S[-1], Y[-1]) / torch.dot(Y[-1], Y[-1]))
            q *= gamma
        else:
            gn = float(torch.linalg.vector_norm(g))
            q *= 1.0 / max(gn, 1e-12)
        for a, rho, s, yv in reversed(alphas):
            bcoef = rho * float(torch.dot(yv, q))
            q += s * (a - bcoef)
        d = -q
        gd = float(torch.dot(g, d))
        if gd >= 0:         # not a descent direction: reset memory
            S, Y = [], []
            d = -g
            gd = float(torch.dot(g, d))
        step = 1.0
        new_loss, new_g = fg(theta + step * d)
        for _ in range(30):     # Armijo backtracking
            if new_loss <= loss + 1e-4 * step * gd:
                break
            step *= 0.5
            new_loss, new_g = fg(theta + step * d)
        s_vec = step * d
        y_vec = new_g - g
        if float(torch.dot(s_vec, y_vec)) > 1e-12:
            S.append(s_vec)
            Y.append(y_vec)
            if len(S) > history_size:
                S.pop(0)
                Y.pop(0)
        theta = theta + s_vec
        improvement = (loss - new_loss) / max(abs(new_loss), abs(loss), 1e-12)
        loss, g = new_loss, new_g
        history.append(loss)
        if abs(improvement) < tol or float(torch.linalg.vector_norm(g)) < 1e-9:
            break
    return theta, history


def train_logistic_regression(features, labels, weights=None, max_iter: int = 100, tol: float = 1e-6,
                              reg_param: float = 0.0, elastic_net: float = 0.0, fit_intercept: bool = True,
                              standardization: bool = True, device=None, history_size: int = 10):
    if not 0.0 <= elastic_net <= 1.0:
        raise ValueError(f"elastic_net must be in [0, 1], got {elastic_net}")
    if reg_param < 0:
        raise ValueError(f"reg_param must be >= 0, got {reg_param}")
    dev = torch.device(device) if device is not None else default_device()
    vc = features if isinstance(features, VectorColumn) else VectorColumn.from_rows(list(features))
    vc = vc.to(dev)
    indptr, idx, val = vc.csr()
    idx = idx.to(torch.int32).contiguous()
    val = val.to(torch.float64).contiguous()
    F = vc.size
    n = len(vc)
    y = torch.as_tensor(labels if isinstance(labels, (torch.Tensor, np.ndarray)) else
                        np.asarray([float(v) for v in labels])).to(device=dev, dtype=torch.float64)
    w = torch.ones(n, dtype=torch.float64, device=dev) if weights is None else \
        torch.as_tensor(np.asarray(weights, dtype=np.float64)).to(dev)
    coll = Collectives()
    wsum = float(coll.sum(w.sum().reshape(1))[0])
    t_indptr, t_idx, t_val = transpose_csr(indptr, idx, val, F)

    def xt(v: torch.Tensor, vals: Optional[torch.Tensor] = None) -> torch.Tensor:     # X^T v, fixed order
        return spmv(t_indptr, t_idx, t_val if vals is None else vals, v)

    scale = _feature_scale(xt, t_val, w, wsum, coll, F, standardization)

    def fg(theta: torch.Tensor):
        beta, b = theta[:F], theta[F]
        m = spmv(indptr, idx, val, scale * beta) + (b if fit_intercept else 0.0)
        # stable log(1 + e^m) - y m
        loss_i = torch.clamp(m, min=0) - m * y + torch.log1p(torch.exp(-torch.abs(m)))
        r = w * (torch.sigmoid(m) - y)
        parts = torch.cat([(w * loss_i).sum().reshape(1), r.sum().reshape(1), xt(r)])
        parts = coll.sum(parts)
        loss = parts[0] / wsum + 0.5 * reg_param * torch.dot(beta, beta)
        g = torch.empty_like(theta)
        g[:F] = scale * parts[2:] / wsum + reg_param * beta
        g[F] = parts[1] / wsum if fit_intercept else 0.0
        return float(loss), g

    theta = torch.zeros(F + 1, dtype=torch.float64, device=dev)
    if fit_intercept:
        p = float(coll.sum((w * y).sum().reshape(1))[0]) / wsum
        if 0 < p < 1:
            theta[F] = math.log(p / (1 - p))
    if reg_param > 0 and elastic_net > 0:
        return _train_owlqn((indptr, idx, val), (t_indptr, t_idx, t_val), y, w, wsum, scale, theta, coll,
                            reg_param * elastic_net, reg_param * (1.0 - elastic_net), max_iter, tol, fit_intercept,
                            history_size)
    theta, history = _lbfgs(fg, theta, max_iter, tol, history_size)
    coef = (scale * theta[:F]).cpu().numpy()
    intercept = float(theta[F]) if fit_intercept else 0.0
    return coef, intercept, history


# counters of the last OWL-QN fit (evaluations = line-search trials + 1, host reads, iterations):
# read by the profile note and the micro-benchmark, never by the trainer itself
OWLQN_STATS = {"evaluations": 0, "host_reads": 0, "iterations": 0}


class OwlqnEvaluation:
    """One function evaluation of the elastic-net objective on a row shard, all on the device:
    ``lr_owlqn_step`` (trial point ``pi(x + t d; xi)``, its norms and ``pg . (x_new - x)``),
    ``lr_forward`` (residuals, loss and residual sums), the transposed SpMV, one ``coll.sum`` of
    ``[loss, sum r, X^T r]`` and ``lr_pseudo_grad``."""

    def __init__(self, csr, t_csr, y, w, wsum, scale, coll, l1, l2, fit_intercept):
        self.csr, self.t_csr, self.y, self.w, self.wsum, self.scale, self.coll = csr, t_csr, y, w, wsum, scale, coll
        self.l1, self.l2, self.fit_intercept = l1, l2, fit_intercept

    def __call__(self, x, d, xi, pg, t: float):
        """Returns ``(x_new, xs_new, g, pg_new, xi_new, |pg_new|^2)`` and the device tuple
        ``[objective, pg . (x_new - x), |pg_new|^2]`` the line search reads."""
        F = self.scale.numel()
        x_new, xs_new, norms = lr_owlqn_step(x, d, xi, pg, self.scale, t)
        parts = torch.empty(F + 2, dtype=torch.float64, device=x.device)
        r, _ = lr_forward(*self.csr, xs_new, x_new[F:], self.y, self.w, out=parts[:2])
        native.lib().spmv(*self.t_csr, r, parts[2:], 0)
        parts = self.coll.sum(parts)
        g, pg_new, xi_new, pgn2 = lr_pseudo_grad(parts, self.scale, x_new, self.wsum, self.l1, self.l2,
                                                 self.fit_intercept)
        obj = parts[0] / self.wsum + (0.5 * self.l2) * norms[1] + self.l1 * norms[0]
        return (x_new, xs_new, g, pg_new, xi_new, pgn2), torch.stack([obj, norms[2], pgn2[0]])


def _train_owlqn(csr, t_csr, y, w, wsum, scale, theta, coll, l1, l2, max_iter, tol, fit_intercept, history_size):
    """OWL-QN (Andrew & Gao 2007) on ``mean log-loss + l2/2 |beta|^2 + l1 |beta|_1`` over the coefficients
    ``theta[:F]`` the optimiser sees (``scale`` maps them to raw-feature coefficients); ``theta[F]`` is
    the unpenalised intercept. The two-loop recursion runs on 0-dim device tensors; the host reads
    one tuple per line-search trial (objective, ``pg . (x_new - x)``, ``|pg|^2``) and one per iteration
    (``s . y``)."""
    dev = theta.device
    F = theta.numel() - 1
    evaluation = OwlqnEvaluation(csr, t_csr, y, w, wsum, scale, coll, l1, l2, fit_intercept)
    pinned = torch.empty(3, dtype=torch.float64, pin_memory=dev.type == "cuda")
    stats = OWLQN_STATS
    stats.update(evaluations=0, host_reads=0, iterations=0)

    def read(values: torch.Tensor) -> list:
        stats["host_reads"] += 1
        if dev.type != "cuda":
            return values.tolist()
        pinned[:values.numel()].copy_(values, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return pinned[:values.numel()].tolist()

    def evaluate(x, d, xi, pg, t):
        stats["evaluations"] += 1
        state, packed = evaluation(x, d, xi, pg, t)
        f, dec, gn2 = read(packed)
        return state, f, dec, gn2

    penalised = torch.ones(F + 1, dtype=torch.bool, device=dev)
    penalised[F] = False

    def aligned(d, pg):     # coefficients move only against their pseudo-gradient
        return torch.where(penalised & (d * pg >= 0), torch.zeros_like(d), d)

    zero = torch.zeros_like(theta)
    # x0 has no non-zero coefficient, so the projection onto the orthant xi = 0 leaves it as it is
    (x, xs, g, pg, xi, pgn2), f, _, gn2 = evaluate(theta, zero, zero, zero, 0.0)
    history = [f]
    S, Y, RHO = [], [], []
    gamma = None
    for _ in range(max_iter):
        if math.sqrt(gn2) < 1e-9:
            break
        stats["iterations"] += 1
        q = pg.clone()
        alphas = []
        for s, yv, rho in zip(reversed(S), reversed(Y), reversed(RHO)):
            a = rho * torch.dot(s, q)
            alphas.append(a)
            q.addcmul_(yv, a, value=-1.0)
        if S:
            q *= gamma
        else:
            q *= 1.0 / torch.clamp(torch.sqrt(pgn2[0]), min=1e-12)
        for s, yv, rho, a in zip(S, Y, RHO, reversed(alphas)):
            q.addcmul_(s, a - rho * torch.dot(yv, q))
        d = aligned(-q, pg)
        step, accepted = 1.0, None
        trials = 0
        while trials < 30:
            trials += 1
            new, f_new, dec, gn2_new = evaluate(x, d, xi, pg, step)
            if dec < 0 and f_new <= f + 1e-4 * dec:
                accepted = new
                break
            if dec >= 0 and S:          # not a descent direction: reset memory, restart the search
                S, Y, RHO = [], [], []
                d = aligned(-pg / torch.clamp(torch.sqrt(pgn2[0]), min=1e-12), pg)
                step, trials = 1.0, 0
                continue
            step *= 0.5
        if accepted is None:            # no decrease along the steepest pseudo-gradient direction
            break
        x_new, xs_new, g_new, pg_new, xi_new, pgn2_new = accepted
        s_vec, y_vec = x_new - x, g_new - g
        sy = torch.dot(s_vec, y_vec)
        if read(sy.reshape(1))[0] > 1e-12:
            S.append(s_vec)
            Y.append(y_vec)
            RHO.append(1.0 / sy)
            gamma = sy / torch.dot(y_vec, y_vec)
            if len(S) > history_size:
                S.pop(0)
                Y.pop(0)
                RHO.pop(0)
        improvement = (f - f_new) / max(abs(f_new), abs(f), 1e-12)
        x, xs, g, pg, xi, pgn2, f, gn2 = x_new, xs_new, g_new, pg_new, xi_new, pgn2_new, f_new, gn2_new
        history.append(f)
        if abs(improvement) < tol:
            break
    coef = xs.cpu().numpy()        # scale * x[:F]: a coefficient left at exactly 0.0 stays 0.0
    intercept = float(x[F]) if fit_intercept else 0.0
    return coef, intercept, history


# ============================================================================ multinomial
def label_maximum(labels, device=None) -> float:
    """Largest label over all ranks (one MAX all-reduce under data parallelism): ``family="auto"``
    is multinomial iff it exceeds 1."""
    y = torch.as_tensor(labels if isinstance(labels, (torch.Tensor, np.ndarray)) else
                        np.asarray([float(v) for v in labels])).to(torch.float64).reshape(-1)
    m = y.max().reshape(1) if y.numel() else y.new_zeros(1)
    if D.is_dist():
        m = D.all_reduce_max(m.to(torch.device(device) if device is not None else default_device()))
    return float(m[0])


# counters of the last multinomial fit: read by the profile note and the micro-benchmark only
MLR_STATS = {"evaluations": 0, "iterations": 0, "k": 0, "kl": 0}


def train_multinomial_logistic_regression(features, labels, weights=None, max_iter: int = 100, tol: float = 1e-6,
                                          reg_param: float = 0.0, elastic_net: float = 0.0,
                                          fit_intercept: bool = True, standardization: bool = True, device=None,
                                          history_size: int = 10, hot=None, chunk_rows: int = 0, threads: int = 0):
    """Spark's multinomial ``LogisticRegression`` with an L2 penalty: minimises
    ``(1/W) sum_i w_i [logsumexp_c(m_ic) - m_{i, y_i}] + regParam/2 |B|_F^2`` with
    ``m_ic = b_c + sum_j x_ij s_j B_cj`` by the L-BFGS loop of the binomial route on ``[B.ravel(), b]``.
    One evaluation is one fused ``ops.sparse.mlr_eval`` pass whose reduced quantities are exact int64
    sums, so for given residuals the gradient and the loss depend on no order of summation; under data
    parallelism an evaluation all-reduces that one int64 block. Labels are integers in ``0 .. C - 1``
    with ``C = max label + 1`` (2 .. 8). Returns ``(coefficientMatrix [C, F], interceptVector [C],
    objective history)``; the coefficients are centred over the classes when ``regParam == 0`` and the
    intercepts always, as Spark does. ``hot`` (feature ids summed in LDS on the device, ``None`` =
    ``nb_hot_set``), ``chunk_rows`` and ``threads`` change the speed only."""
    if not 0.0 <= elastic_net <= 1.0:
        raise ValueError(f"elastic_net must be in [0, 1], got {elastic_net}")
    if reg_param < 0:
        raise ValueError(f"reg_param must be >= 0, got {reg_param}")
    if reg_param > 0 and elastic_net > 0:
        raise NotImplementedError("multinomial logistic regression supports elasticNetParam = 0 only "
                                  "(no L1 part)")
    dev, vc, y, w, n = coerce_rows(features, labels, weights, device)
    indptr, idx, val = sparse_csr(vc)
    F = int(vc.size)
    (ymax, ymin_neg, wmax, wmin_neg, vmax), n_global = reduce_statistics(signed_extremes(y, w, val, n), n, dev)
    lim = mlr_limits()
    if not (math.isfinite(ymax) and math.isfinite(ymin_neg)) or ymin_neg > 0 or ymax != math.floor(ymax):
        raise ValueError("multinomial logistic regression labels must be integers in 0 .. C - 1")
    C = max(int(ymax) + 1, 2)
    if C > lim["max_classes"]:
        raise ValueError(f"multinomial logistic regression supports at most {lim['max_classes']} classes, "
                         f"the labels name {C}")
    if not (math.isfinite(wmax) and math.isfinite(wmin_neg)) or wmin_neg > 0:
        raise ValueError("multinomial logistic regression weights must be finite and >= 0")
    if not math.isfinite(vmax):
        raise ValueError("multinomial logistic regression requires finite feature values")
    k, kl = mlr_scale_exponents(wmax, vmax, n_global)
    coll, w_rows, wsum, scale = weight_sum_and_scale(indptr, idx, val, F, w, n, standardization,
                                                     "multinomial logistic regression")
    class_w = coll.sum(torch.stack([(w_rows * (y == c)).sum() for c in range(C)]))
    tables = hot_tables(indptr, idx, val, F, C, hot)
    inv_k = math.ldexp(1.0, -k)
    stats_ = MLR_STATS
    stats_.update(evaluations=0, iterations=0, k=k, kl=kl)

    def fg(theta: torch.Tensor):
        B, b = theta[:C * F].view(C, F), theta[C * F:]
        XS = (scale.unsqueeze(1) * B.t()).contiguous()
        res = mlr_eval(indptr, idx, val, XS, b.contiguous(), y, w, k, kl, tables, chunk_rows=chunk_rows,
                       check_extents=stats_["evaluations"] == 0, threads=threads)
        block = coll.sum(res.block)
        tail = block[-2:].cpu()
        lossq, flag = int(tail[0]), int(tail[1])
        if flag >> 32:
            _raise_bad_input("mlr", idx, val, y, w, F, C)
        first = stats_["evaluations"] == 0
        stats_["evaluations"] += 1
        g = torch.empty_like(theta)
        G = block[:F * C].view(F, C).to(torch.float64) * inv_k
        g[:C * F].view(C, F).copy_(scale.unsqueeze(0) * G.t() / wsum + reg_param * B)
        if fit_intercept:
            g[C * F:] = block[F * C:F * C + C].to(torch.float64) * inv_k / wsum
        else:
            g[C * F:] = 0.0
        if flag & 0xFFFFFFFF:       # a clamped row loss: the trial is rejected like an infinite objective
            if first:
                raise ValueError("multinomial logistic regression: a row's loss at the starting point is not "
                                 f"below {int(lim['loss_cap'])} (margins out of range)")
            return math.inf, g
        loss = math.ldexp(float(lossq), -kl) / wsum + 0.5 * reg_param * float(torch.dot(theta[:C * F], theta[:C * F]))
        return loss, g

    theta = torch.zeros(C * F + C, dtype=torch.float64, device=dev)
    if fit_intercept:
        cw = class_w.cpu().numpy()
        present = cw > 0
        with np.errstate(divide="ignore"):
            lp = np.log(cw / wsum)
        lp[~present] = lp[present].min() - 1.0
        theta[C * F:] = torch.from_numpy(lp - lp[present].mean()).to(dev)
    theta, history = _lbfgs(fg, theta, max_iter, tol, history_size)
    stats_["iterations"] = len(history) - 1
    B = theta[:C * F].view(C, F).cpu().numpy().copy()
    b = theta[C * F:].cpu().numpy().copy()
    if fit_intercept:
        b -= b.mean()
    else:
        b[:] = 0.0
    if reg_param == 0:
        B -= B.mean(axis=0, keepdims=True)
    coef = scale.cpu().numpy()[None, :] * B
    return coef, b, history
