"""Naive Bayes trainer (Spark ``NaiveBayes``, multinomial and Bernoulli): one pass over the data.

The fit is one ``ops.sparse.nb_sums`` pass (``csrc/nb_kernels.hip`` / ``nb_cpu.cpp``): every term
``t_ij = w_i x_ij`` is scaled by ``2^k`` and rounded once to an integer, and the class-conditional
sums are exact int64 sums. Integer adds commute, so host fits, device fits and every world size give
the same sums bit for bit; ``finalize`` below is the only place a logarithm is taken, so they also
give the same model. Under data parallelism (an ambient process group, as for logistic regression)
each rank holds a row shard: the maxima that fix ``k`` are all-reduced with MAX, then one
all-reduce sums the int64 block of ``C F + 2 C`` values.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops.sparse import nb_limits, nb_scale_exponent, nb_sums
from ..parallel import dist as D
from ._linear_common import coerce_rows, reduce_statistics

MODEL_TYPES = ("multinomial", "bernoulli")


def check_model_type(model_type: str) -> str:
    if model_type in ("complement", "gaussian"):
        raise NotImplementedError(f"{model_type} Naive Bayes is not supported (multinomial and bernoulli are)")
    if model_type not in MODEL_TYPES:
        raise ValueError(f"unknown Naive Bayes modelType {model_type!r}")
    return model_type


def _exact_total(q: np.ndarray) -> int:
    """Sum of int64 values as a Python integer (split words: no int64 overflow)."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    return (int((q >> 32).sum()) << 32) + int((q & 0xFFFFFFFF).sum())


def finalize(S, Wq, k: int, kw: int, smoothing: float, model_type: str = "multinomial"):
    """``(pi [C], theta [C, F])`` from the exact sums: ``S`` [C, F] and ``Wq`` [C] int64 with their
    scale exponents. Every path (host, device, every world size) ends here."""
    check_model_type(model_type)
    S = np.asarray(S, dtype=np.int64)
    Wq = np.asarray(Wq, dtype=np.int64)
    C, F = S.shape
    lam = float(smoothing)
    with np.errstate(divide="ignore"):
        n = np.ldexp(Wq.astype(np.float64), -kw)
        total = math.ldexp(float(_exact_total(Wq)), -kw)
        pi = np.log(n + lam) - np.log(total + C * lam)
        num = np.log(np.ldexp(S.astype(np.float64), -k) + lam)
        if model_type == "multinomial":
            T = np.array([math.ldexp(float(_exact_total(S[c])), -k) for c in range(C)])
            den = np.log(T + F * lam)
        else:
            den = np.log(n + 2.0 * lam)
        theta = num - den[:, None]
    return pi, theta


def class_linear(pi: np.ndarray, theta: np.ndarray, model_type: str = "multinomial"):
    """The model as ``C`` linear scores: ``(W [F, C], b [C])`` with ``raw = x W + b``. Multinomial:
    ``W = theta^T, b = pi``. Bernoulli: ``W = (theta - log1p(-exp(theta)))^T`` and
    ``b_c = pi_c + fsum_f log1p(-exp(theta_cf))``."""
    check_model_type(model_type)
    pi = np.asarray(pi, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    if model_type == "multinomial":
        return np.ascontiguousarray(theta.T), pi.copy()
    with np.errstate(divide="ignore"):
        neg = np.log1p(-np.exp(theta))
    b = np.array([pi[c] + math.fsum(neg[c]) for c in range(pi.size)])
    return np.ascontiguousarray((theta - neg).T), b


def fit_naive_bayes(features, labels, weights=None, smoothing: float = 1.0, model_type: str = "multinomial",
                    device=None, hot=None, threads: int = 0) -> dict:
    """Fit on a ``VectorColumn`` (rows of this rank under data parallelism). Returns ``pi`` [C],
    ``theta`` [C, F], ``C``, ``F`` and, for the record, the scale exponents ``k`` / ``kw`` and the row
    count per class ``cnt``."""
    check_model_type(model_type)
    if not float(smoothing) >= 0.0:
        raise ValueError(f"smoothing must be >= 0, got {smoothing}")
    bernoulli = model_type == "bernoulli"
    dev, vc, y, w, n = coerce_rows(features, labels, weights, device)
    val = vc.csr()[2]
    # (largest label, largest weight, largest value)
    (ymax, wmax, vmax), n_global = reduce_statistics(
        [y.max() if n else y.new_zeros(()), w.max() if w is not None and n else y.new_ones(()),
         val.max().to(torch.float64) if val.numel() else y.new_zeros(())], n, dev)
    lim = nb_limits()
    if not math.isfinite(ymax) or ymax < 0 or ymax != math.floor(ymax):
        raise ValueError("Naive Bayes labels must be integers in 0 .. C - 1")
    C = max(int(ymax) + 1, 2)
    if C > lim["max_classes"]:
        raise ValueError(f"Naive Bayes supports at most {lim['max_classes']} classes, the labels name {C}")
    if not math.isfinite(wmax) or wmax <= 0:
        raise ValueError("Naive Bayes weights must be finite and > 0")
    if not math.isfinite(vmax):
        raise ValueError("Naive Bayes requires finite feature values")
    k = nb_scale_exponent(wmax * max(vmax, 0.0), n_global)
    kw = nb_scale_exponent(wmax, n_global)
    S, Wq, cnt = nb_sums(vc, y, w, C, k, kw, bernoulli=bernoulli, hot=hot, threads=threads)
    if D.is_dist():
        block = D.all_reduce_sum(torch.cat([S.reshape(-1), Wq, cnt]).to(dev)).cpu()
        F = vc.size
        S, Wq, cnt = block[:C * F].view(C, F), block[C * F:C * F + C], block[C * F + C:]
    pi, theta = finalize(S.numpy(), Wq.numpy(), k, kw, smoothing, model_type)
    return {"pi": pi, "theta": theta, "C": C, "F": int(vc.size), "k": k, "kw": kw, "cnt": cnt.numpy().copy()}
