"""Multinomial logistic regression: the fused fixed-point evaluation (``ops.sparse.mlr_eval``) against
a NumPy / integer statement of its contract, the trainer against SciPy and scikit-learn at the
optimum, the ML API, the Spark layout, serving, determinism and data parallelism."""
import functools
import math
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.models import lr as LR
from fraud_detection_spark_kafka_llm_amd.ops import sparse
from fraud_detection_spark_kafka_llm_amd.ops.text import ClassLinearScorer

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
F = 2048
LIM = sparse.mlr_limits()
CHUNK = LIM["chunk_rows"]
MAXC = LIM["max_classes"]
EDGE_LENS = [0, 1, 63, 64, 65, 129]
FORCED = [40.0, -40.0, 800.0, -800.0]           # margins of class 0 in single-entry rows
# error of mlr_eval's per-row terms against the NumPy fp64 formula, |r - r_np| / w and
# |loss - loss_np| / max(1, max_c |m_c|): 4 x the largest value measured on the MI355X over the cases
# of this file (5.921e-16 for r, 4.441e-16 for the loss, profiles/r15/multinomial_lr.md), never above 1e-13
ROW_TERM_TOL = min(4 * 5.921e-16, 1e-13)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---------------------------------------------------------------------------------------------- corpus
def corpus(n, C, dtype_name, weighted, seed=5, integer=False):
    """CSR of ``n`` rows (the edge lengths first, frequent and rare features, some negative values),
    labels, weights from {0.5, 3.0} or None, and a parameter point ``(XS [F, C], b [C])``. The first
    ``len(FORCED)`` features carry the forced margins: the single-entry rows that follow the edge rows."""
    rng = np.random.default_rng(seed)
    lens = (EDGE_LENS + [1] * len(FORCED) + list(rng.integers(0, 40, size=max(0, n))))[:n]
    ptr, idx, val = [0], [], []
    pool = np.arange(len(FORCED), F)
    p = 1.0 / (1.0 + np.arange(pool.size)) ** 0.9
    p /= p.sum()
    for i, m in enumerate(lens):
        forced = len(EDGE_LENS) <= i < len(EDGE_LENS) + len(FORCED)
        ids = np.array([i - len(EDGE_LENS)]) if forced else rng.choice(pool, size=m, replace=False, p=p)
        v = rng.integers(1, 6, size=m).astype(np.float64) if integer else rng.random(m) * 3 + 0.1
        v = np.where(rng.random(m) < 0.15, -v, v)
        idx.append(ids.astype(np.int32))
        val.append(np.ones(1) if forced else v)
        ptr.append(ptr[-1] + m)
    csr = (np.asarray(ptr, dtype=np.int64), np.concatenate(idx).astype(np.int32),
           np.concatenate(val).astype(dtype_name))
    y = rng.integers(0, C, size=n).astype(np.float64)
    w = rng.choice([0.5, 3.0], size=n) if weighted else None
    XS = rng.normal(0, 0.4, size=(F, C))
    XS[:len(FORCED)] = 0.0
    XS[:len(FORCED), 0] = FORCED
    return csr, y, w, XS, rng.normal(0, 0.5, size=C)


def to_vc(csr, dev, size=F) -> VectorColumn:
    ip, ix, v = csr
    return VectorColumn(size, torch.from_numpy(ip).to(dev), torch.from_numpy(ix).to(dev), torch.from_numpy(v).to(dev))


def run_eval(csr, y, w, XS, b, dev, k=None, kl=None, hot=None, want_rows=True, **kw):
    """``mlr_eval`` at the exponents of the data; ``hot``: None = the default hot set, else feature ids."""
    ip, ix, v = (torch.from_numpy(a).to(dev) for a in csr)
    C = XS.shape[1]
    if k is None:
        k, kl = sparse.mlr_scale_exponents(3.0 if w is not None else 1.0, float(np.abs(csr[2]).max(initial=0.0)), len(y))
    tables = (None, None)
    if torch.device(dev).type == "cuda":
        feat = sparse.nb_hot_set(ip, ix, v, XS.shape[0], C) if hot is None else torch.as_tensor(hot, dtype=torch.int32, device=dev)
        tables = sparse.nb_hot_tables(feat, XS.shape[0], C)
    res = sparse.mlr_eval(ip, ix, v, torch.from_numpy(XS).to(dev), torch.from_numpy(b).to(dev),
                          torch.from_numpy(y).to(dev), None if w is None else torch.from_numpy(w).to(dev), k, kl,
                          tables, want_rows=want_rows, **kw)
    return res, k, kl


def quant(t, k) -> np.ndarray:
    return np.rint(np.ldexp(np.asarray(t, dtype=np.float64), k)).astype(np.int64)


def integer_oracle(csr, w, R, loss_row, k, kl, C, size=F):
    """The block as exact integer sums of ``rint(ldexp(., k))`` of the given residuals and losses."""
    ip, ix, v = csr
    row_of = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    G = np.zeros((size, C), dtype=np.int64)
    np.add.at(G, ix, quant(v.astype(np.float64)[:, None] * R[row_of], k))
    gb = [sum(int(q) for q in quant(R[:, c], k)) for c in range(C)]
    ww = np.ones(len(loss_row)) if w is None else w
    return G, np.array(gb, dtype=np.int64), sum(int(q) for q in quant(ww * loss_row, kl))


def numpy_row_terms(m, y, w):
    mx = m.max(axis=1, keepdims=True)
    e = np.exp(m - mx)
    S = e.sum(axis=1, keepdims=True)
    onehot = np.arange(m.shape[1])[None, :] == y.astype(np.int64)[:, None]
    loss = (mx[:, 0] - m[onehot]) + np.log(S[:, 0])
    return (1.0 if w is None else w[:, None]) * (e / S - onehot), loss


def check_eval(csr, y, w, XS, b, dev, **kw):
    """Every per-evaluation assertion of the contract; returns the block and the row-term errors."""
    C = XS.shape[1]
    res, k, kl = run_eval(csr, y, w, XS, b, dev, **kw)
    block = res.block.cpu().numpy()
    margin, R, loss_row = (t.cpu().numpy() for t in (res.margin, res.R, res.loss_row))
    want = sparse.score_csr(to_vc(csr, dev), ClassLinearScorer(XS, b)).cpu().numpy()
    assert np.array_equal(bits(margin), bits(want))
    G, gb, lq = integer_oracle(csr, w, R, loss_row, k, kl, C)
    assert np.array_equal(block[:F * C].reshape(F, C), G)
    assert np.array_equal(block[F * C:F * C + C], gb) and int(block[-2]) == lq and int(block[-1]) == 0
    assert not res.clamped and not res.bad_input
    r_np, loss_np = numpy_row_terms(margin, y, w)
    ww = 1.0 if w is None else w[:, None]
    err_r = float(np.max(np.abs(R - r_np) / ww, initial=0.0))
    err_l = float(np.max(np.abs(loss_row - loss_np) / np.maximum(1.0, np.abs(margin).max(axis=1)), initial=0.0))
    print(f"{dev} rows={len(y)} C={C} {csr[2].dtype}: row-term error r {err_r:.3e} loss {err_l:.3e}")
    assert err_r <= ROW_TERM_TOL and err_l <= ROW_TERM_TOL
    assert np.all(np.abs(R) <= (1.0 if w is None else w[:, None])) and np.all(loss_row >= 0)
    return block, (k, kl), (margin, R, loss_row)


# ---------------------------------------------------------------------------------------------- 1. kernel = contract
def test_limits_are_exported():
    assert LIM["max_classes"] == sparse.nb_limits()["max_classes"] == 8 and LIM["loss_cap"] == 2.0 ** LIM["loss_bits"] == 2048
    assert LIM["flag_clamped"] == 1 and LIM["flag_bad_input"] == 1 << 32 and CHUNK == 1024


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_block_equals_the_integer_oracle_around_the_row_chunk(n, dev):
    csr, y, w, XS, b = corpus(n, 3, "float32", True, seed=n)
    check_eval(csr, y, w, XS, b, dev)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_block_equals_the_integer_oracle(C, dtype_name, weighted, dev):
    csr, y, w, XS, b = corpus(CHUNK + 1, C, dtype_name, weighted)
    _, _, (margin, R, loss_row) = check_eval(csr, y, w, XS, b, dev)
    forced = slice(len(EDGE_LENS), len(EDGE_LENS) + len(FORCED))
    assert np.array_equal(margin[forced, 0], np.asarray(FORCED) + b[0])
    assert np.all(np.isfinite(R)) and np.all(loss_row < 2048)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_hot_set_chunk_and_threads_change_no_bit(C, dev):
    csr, y, w, XS, b = corpus(2 * CHUNK + 1, C, "float32", True, seed=9)
    ref, (k, kl), _ = check_eval(csr, y, w, XS, b, dev)
    slots = LIM["max_table_bytes"] // (8 * C)
    for kw in (dict(hot=[]), dict(hot=list(range(min(F, slots)))), dict(chunk_rows=1), dict(chunk_rows=7),
               dict(threads=1), dict(threads=7)):
        res, _, _ = run_eval(csr, y, w, XS, b, dev, k=k, kl=kl, want_rows=False, **kw)
        assert np.array_equal(res.block.cpu().numpy(), ref), kw
    # a host block and a device block agree through the oracle: each equals the integer sums of its own residuals
    host, _, _ = check_eval(csr, y, w, XS, b, "cpu")
    if dev != "cpu":
        print(f"device block == host block: {np.array_equal(host, ref)}")


@pytest.mark.parametrize("dev", DEVICES)
def test_gradient_is_within_half_a_unit_per_stored_entry_of_the_exact_sum(dev):
    C = 3
    csr, y, w, XS, b = corpus(200, C, "float64", True, seed=21)
    block, (k, _), (_, R, _) = check_eval(csr, y, w, XS, b, dev)
    ip, ix, v = csr
    row_of = np.repeat(np.arange(len(y)), np.diff(ip))
    exact = {}
    for j in range(len(ix)):
        for c in range(C):
            key = (int(ix[j]), c)
            exact[key] = exact.get(key, Fraction(0)) + Fraction(float(v[j]) * float(R[row_of[j], c]))
    df = np.bincount(ix, minlength=F)
    G = block[:F * C].reshape(F, C)
    worst = Fraction(0)
    for (f, c), want in exact.items():
        gap = abs(Fraction(int(G[f, c]), 2 ** k) - want)
        assert gap <= Fraction(int(df[f]), 2 ** (k + 1))
        worst = max(worst, gap / Fraction(int(df[f]), 2 ** (k + 1)))
    print(f"largest gradient gap / (df 2^-(k+1)) = {float(worst):.3f}, k = {k}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, MAXC])
def test_integer_values_and_dyadic_residuals_sum_exactly(C, dev):
    """With all margins equal p_c = 1 / C is exact for C a power of two, so every term is dyadic."""
    csr, y, w, _, _ = corpus(CHUNK + 9, C, "float32", True, seed=4, integer=True)
    block, (k, _), (_, R, _) = check_eval(csr, y, w, np.zeros((F, C)), np.zeros(C), dev)
    onehot = np.arange(C)[None, :] == y.astype(np.int64)[:, None]
    assert np.array_equal(R, w[:, None] * (1.0 / C - onehot))
    ip, ix, v = csr
    row_of = np.repeat(np.arange(len(y)), np.diff(ip))
    want = np.zeros((F, C))
    np.add.at(want, ix, v.astype(np.float64)[:, None] * R[row_of])        # dyadic terms: fp64 adds are exact
    assert np.array_equal(np.ldexp(block[:F * C].reshape(F, C).astype(np.float64), -k), want)
    assert np.array_equal(np.ldexp(block[F * C:F * C + C].astype(np.float64), -k), R.sum(axis=0))


def test_scale_exponents_follow_the_formula():
    kmax, bits_ = LIM["k_max"], LIM["sum_bits"]
    assert sparse.mlr_scale_exponents(1.0, 1.0, 2 ** 20 - 1) == (min(kmax, bits_ - 20 - 1), bits_ - 20 - 1 - 11)
    assert sparse.mlr_scale_exponents(1.0, 1.0, 2 ** 20) == (min(kmax, bits_ - 21 - 1), bits_ - 21 - 1 - 11)
    assert sparse.mlr_scale_exponents(1.0, 0.25, 2 ** 20) == sparse.mlr_scale_exponents(1.0, 1.0, 2 ** 20)
    assert sparse.mlr_scale_exponents(3.0, 4000.5, 1025) == (bits_ - 11 - 14, min(kmax, bits_ - 11 - 2 - 11))
    assert sparse.mlr_scale_exponents(0.5, 2.0 ** 20, 1000)[0] == bits_ - 10 - 20
    with pytest.raises(ValueError, match="do not fit the exact 61-bit sums of multinomial"):
        sparse.mlr_scale_exponents(1.0, 2.0 ** 45, 2 ** 20)
    with pytest.raises(ValueError, match="finite"):
        sparse.mlr_scale_exponents(float("nan"), 1.0, 10)
    with pytest.raises(ValueError, match="Naive Bayes"):                # the sibling keeps its own text
        sparse.nb_scale_exponent(float("nan"), 10)


@pytest.mark.parametrize("dev", DEVICES)
def test_a_loss_of_5000_is_clamped_and_flagged(dev):
    C = 3
    csr, y, w, XS, b = corpus(40, C, "float64", True, seed=2)
    XS[0, 0], b[:] = 5000.0, 0.0
    row = len(EDGE_LENS)                        # the single-entry row on feature 0
    y[row] = 1.0
    res, k, kl = run_eval(csr, y, w, XS, b, dev)
    assert res.clamped and not res.bad_input and int(res.block[-1]) == LIM["flag_clamped"]
    R, loss_row = res.R.cpu().numpy(), res.loss_row.cpu().numpy()
    assert loss_row[row] == 2048.0 and np.all(np.delete(loss_row, row) < 2048)
    assert np.array_equal(R[row], w[row] * np.array([1.0, -1.0, 0.0]))
    G, gb, lq = integer_oracle(csr, w, R, loss_row, k, kl, C)
    block = res.block.cpu().numpy()
    assert np.array_equal(block[:F * C].reshape(F, C), G) and np.array_equal(block[F * C:F * C + C], gb) and int(block[-2]) == lq
    XS[0, 0] = float("inf")                     # a margin that is not finite: clamped, no residual, nothing is NaN
    res, _, _ = run_eval(csr, y, w, XS, b, dev)
    assert res.clamped and np.array_equal(res.R.cpu().numpy()[row], np.zeros(C)) and res.loss_row.cpu().numpy()[row] == 2048.0


@pytest.mark.parametrize("dev", DEVICES)
def test_bad_input_sets_the_second_flag_and_adds_nothing(dev):
    C = 3
    csr, y, w, XS, b = corpus(70, C, "float64", True, seed=8)
    clean, k, kl = run_eval(csr, y, w, XS, b, dev)
    row = 20
    lo = int(csr[0][row])
    assert csr[0][row + 1] > lo

    def without_row():
        y2, w2 = y.copy(), w.copy()
        w2[row] = 0.0                           # a row of weight 0 adds nothing either
        return run_eval(csr, y2, w2, XS, b, dev, k=k, kl=kl)[0].block.cpu().numpy()

    want = without_row()
    for what, bad in [("y", -1.0), ("y", 1.5), ("y", float(C)), ("y", float("nan")), ("w", -0.5), ("w", float("nan")),
                      ("w", float("inf")), ("v", float("nan")), ("v", float("inf")), ("i", F), ("i", -1)]:
        ip, ix, v = csr[0], csr[1].copy(), csr[2].copy()
        y2, w2 = y.copy(), w.copy()
        if what == "y":
            y2[row] = bad
        elif what == "w":
            w2[row] = bad
        elif what == "v":
            v[lo] = bad
        else:
            ix[lo] = bad
        res, _, _ = run_eval((ip, ix, v), y2, w2, XS, b, dev, k=k, kl=kl)
        got = res.block.cpu().numpy()
        assert res.bad_input and not res.clamped, (what, bad)
        assert np.array_equal(got[:-1], want[:-1]), (what, bad)
    assert int(clean.block[-1]) == 0


# ---------------------------------------------------------------------------------------------- 2. optimum
@functools.lru_cache(maxsize=None)
def opt_corpus(C):
    rng = np.random.default_rng(11)
    X = (rng.random((800, 150)) < 0.08) * rng.random((800, 150)) * 4
    groups = np.stack([X[:, 3 * c:3 * c + 3].sum(axis=1) for c in range(C)], axis=1)
    y = np.argmax(groups + rng.normal(0, 0.3, size=(800, C)), axis=1).astype(np.float64)
    X.setflags(write=False)
    return X, y


def dense_vc(X, dev="cpu") -> VectorColumn:
    return VectorColumn(X.shape[1], dense=torch.from_numpy(np.array(X)).to(dev))


def feature_scale(X, standardization):
    std = X.std(axis=0, ddof=1)
    return np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0) if standardization else np.ones(X.shape[1])


def objective(theta, Xs, y, reg, C):
    """The contract's objective and gradient in the optimiser's coordinates (NumPy fp64)."""
    n, Fx = Xs.shape
    B, b = theta[:C * Fx].reshape(C, Fx), theta[C * Fx:]
    m = Xs @ B.T + b
    mx = m.max(axis=1, keepdims=True)
    e = np.exp(m - mx)
    S = e.sum(axis=1, keepdims=True)
    onehot = np.arange(C)[None, :] == y.astype(np.int64)[:, None]
    f = float(np.mean(mx[:, 0] + np.log(S[:, 0]) - m[onehot])) + 0.5 * reg * float(np.sum(B * B))
    R = (e / S - onehot) / n
    return f, np.concatenate([(R.T @ Xs + reg * B).ravel(), R.sum(axis=0)])


OPT_CASES = [(C, reg, std) for C in (3, 4) for reg, std in ((0.02, True), (0.005, False))]


@functools.lru_cache(maxsize=None)
def reference(C, reg, std):
    from scipy.optimize import minimize

    X, y = opt_corpus(C)
    s = feature_scale(X, std)
    Xs = X * s
    res = minimize(objective, np.zeros(C * X.shape[1] + C), args=(Xs, y, reg, C), jac=True, method="L-BFGS-B",
                   options=dict(maxiter=20000, maxfun=40000, ftol=1e-16, gtol=1e-10, maxcor=30))
    theta = res.x
    Fx = X.shape[1]
    b = theta[C * Fx:]
    return s * theta[:C * Fx].reshape(C, Fx), b - b.mean(), res.fun, theta, Xs


@pytest.mark.parametrize("C,reg,std", OPT_CASES)
def test_reference_is_converged(C, reg, std):
    _, _, _, theta, Xs = reference(C, reg, std)
    g = objective(theta, Xs, opt_corpus(C)[1], reg, C)[1]
    print(f"reference gradient inf-norm {np.abs(g).max():.3e}")
    assert np.abs(g).max() <= 1e-8


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C,reg,std", OPT_CASES)
def test_fit_reaches_the_reference_optimum(C, reg, std, dev):
    X, y = opt_corpus(C)
    coef_ref, b_ref, f_ref, _, Xs = reference(C, reg, std)
    coef, b, hist = LR.train_multinomial_logistic_regression(dense_vc(X, dev), y, reg_param=reg, standardization=std,
                                                             max_iter=500, tol=1e-12, device=dev)
    s = feature_scale(X, std)
    B = np.where(s > 0, coef / np.where(s > 0, s, 1.0), 0.0)
    f, g = objective(np.concatenate([B.ravel(), b]), Xs, y, reg, C)
    print(f"{dev} C={C} reg={reg} std={std}: objective gap {f - f_ref:.3e} coef gap {np.abs(coef - coef_ref).max():.3e} "
          f"intercept gap {np.abs(b - b.mean() - b_ref).max():.3e} gradient {np.abs(g).max():.3e} "
          f"evaluations {LR.MLR_STATS['evaluations']}")
    assert coef.shape == (C, X.shape[1]) and b.shape == (C,)
    assert f <= f_ref + 1e-10
    assert np.abs(coef - coef_ref).max() <= 1e-4 and np.abs(b - b.mean() - b_ref).max() <= 1e-4
    assert np.abs(g).max() <= 1e-5
    assert all(a >= c for a, c in zip(hist, hist[1:]))
    assert abs(hist[-1] - f) <= 1e-9 and LR.MLR_STATS["k"] == 40


@pytest.mark.parametrize("dev", DEVICES)
def test_without_a_penalty_the_model_is_centred(dev):
    X, y = opt_corpus(3)
    coef, b, hist = LR.train_multinomial_logistic_regression(dense_vc(X, dev), y, reg_param=0.0, max_iter=25, device=dev)
    assert np.abs(coef.mean(axis=0)).max() <= 1e-12 * np.abs(coef).max() and abs(b.mean()) <= 1e-12 * np.abs(b).max()
    assert all(a >= c for a, c in zip(hist, hist[1:])) and len(hist) > 5


@pytest.mark.parametrize("dev", DEVICES)
def test_a_clamped_trial_is_rejected_like_an_infinite_objective(dev, monkeypatch):
    """Values of 1e5: the first unit steps move some margin by more than 2048, the pass flags those
    trials, and the line search halves the step as it does for an objective of +inf."""
    X, y = opt_corpus(3)
    clamped = []

    def spy(*a, **kw):
        res = sparse.mlr_eval(*a, **kw)
        clamped.append(res.clamped)
        return res

    monkeypatch.setattr(LR, "mlr_eval", spy)
    coef, b, hist = LR.train_multinomial_logistic_regression(dense_vc(X * 3.0e4, dev), y, reg_param=0.01,
                                                             standardization=False, max_iter=15, device=dev)
    print(f"{dev}: {sum(clamped)} of {len(clamped)} evaluations clamped, objective {hist[0]:.4f} -> {hist[-1]:.4f}")
    assert not clamped[0] and sum(clamped) >= 1 and len(clamped) == LR.MLR_STATS["evaluations"]
    assert np.all(np.isfinite(coef)) and np.all(np.isfinite(b)) and np.all(np.isfinite(hist))
    assert all(a >= c for a, c in zip(hist, hist[1:])) and hist[-1] < 0.5 * hist[0]
    assert LR.MLR_STATS["k"] == 61 - 10 - 17                 # 800 rows, values below 2^17


# ---------------------------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("dev", DEVICES)
def test_two_class_multinomial_is_the_binomial_fit_at_half_the_penalty(dev):
    X, y3 = opt_corpus(3)
    y = (y3 > 0).astype(np.float64)
    r = 0.02
    W, b, _ = LR.train_multinomial_logistic_regression(dense_vc(X, dev), y, reg_param=r, max_iter=500, tol=1e-12, device=dev)
    w1, b1, _ = LR.train_logistic_regression(dense_vc(X, dev), y, reg_param=r / 2, max_iter=500, tol=1e-12, device=dev)
    assert W.shape == (2, X.shape[1])
    print(f"margin gap {np.abs(W[1] - W[0] - w1).max():.3e} {abs(b[1] - b[0] - b1):.3e}, symmetry {np.abs(W[0] + W[1]).max():.3e}")
    assert np.abs(W[1] - W[0] - w1).max() <= 1e-4 and abs(b[1] - b[0] - b1) <= 1e-4
    assert np.abs(W[0] + W[1]).max() <= 1e-9 and abs(b[0] + b[1]) <= 1e-9


@pytest.mark.parametrize("dev", DEVICES)
def test_raw_feature_fit_matches_sklearn(dev):
    from sklearn.linear_model import LogisticRegression as SkLR

    X, y = opt_corpus(3)
    r = 0.01
    sk = SkLR(C=1.0 / (r * len(y)), tol=1e-12, max_iter=20000).fit(X, y)
    W, b, _ = LR.train_multinomial_logistic_regression(dense_vc(X, dev), y, reg_param=r, standardization=False,
                                                       max_iter=500, tol=1e-12, device=dev)
    gap = max(np.abs(W - sk.coef_).max(), np.abs(b - (sk.intercept_ - sk.intercept_.mean())).max())
    print(f"largest gap to scikit-learn {gap:.3e}")
    assert gap <= 1e-4


@pytest.mark.parametrize("dev", DEVICES)
def test_a_class_without_rows_fits_and_never_wins(dev):
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, LogisticRegression

    X, y3 = opt_corpus(3)
    y = np.where(y3 == 2, 3.0, y3)                         # labels 0, 1, 3: class 2 has no rows
    df = Frame({"features": dense_vc(X, dev), "label": y})
    m = LogisticRegression(regParam=0.01, maxIter=60).fit(df)
    assert m.numClasses == 4 and m.coefficientMatrix.shape == (4, X.shape[1]) and np.all(np.isfinite(m.interceptVector))
    out = m.transform(df)
    pred = out.column("prediction").cpu().numpy()
    prob = out.column("probability").cpu().numpy()
    assert not np.any(pred == 2.0) and (pred == y).mean() > 0.8
    assert np.abs(prob.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52


@pytest.mark.parametrize("dev", DEVICES)
def test_bad_input_raises_before_any_model(dev):
    X, y = opt_corpus(3)
    vc = dense_vc(X, dev)
    fit = functools.partial(LR.train_multinomial_logistic_regression, device=dev, max_iter=3)

    def changed(i, v):
        z = y.copy()
        z[i] = v
        return z

    for bad in (1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="labels must be integers"):
            fit(vc, changed(7, bad))
    with pytest.raises(ValueError, match="at most 8 classes"):
        fit(vc, changed(7, 8.0))
    for bad in (-0.5, float("nan"), float("inf")):
        w = np.ones(len(y))
        w[3] = bad
        with pytest.raises(ValueError, match="weights must be finite and >= 0"):
            fit(vc, y, weights=w)
    for bad in (float("nan"), float("inf")):
        Z = X.copy()
        Z[5, 2] = bad
        with pytest.raises(ValueError, match="finite feature values"):
            fit(dense_vc(Z, dev), y)
    with pytest.raises(ValueError, match="one entry per row"):
        fit(vc, y[:-1])
    with pytest.raises(NotImplementedError, match="elasticNetParam = 0 only"):
        fit(vc, y, reg_param=0.02, elastic_net=0.5)
    Z = X.copy()
    Z[5, 2] = -2.5                                          # negative values are legal
    assert fit(dense_vc(Z, dev), y, reg_param=0.01)[0].shape == (3, X.shape[1])


def test_family_routing():
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, LogisticRegression

    X, y = opt_corpus(3)
    df = Frame({"features": dense_vc(X), "label": y})
    with pytest.raises(ValueError, match="family='binomial' needs labels in"):
        LogisticRegression(family="binomial", maxIter=2).fit(df)
    assert LogisticRegression(maxIter=2, regParam=0.01).fit(df).numClasses == 3          # auto
    two = Frame({"features": dense_vc(X), "label": (y > 0).astype(np.float64)})
    auto = LogisticRegression(maxIter=2, regParam=0.01).fit(two)
    assert not auto.isMultinomial and auto.coefficientMatrix.shape == (1, X.shape[1]) and auto.interceptVector.shape == (1,)
    assert np.array_equal(bits(auto.coefficientMatrix[0]), bits(auto.coefficients)) and auto.interceptVector[0] == auto.intercept
    multi = LogisticRegression(family="multinomial", maxIter=2, regParam=0.01).fit(two)
    assert multi.isMultinomial and multi.numClasses == 2 and multi.coefficientMatrix.shape == (2, X.shape[1])
    for name in ("coefficients", "intercept"):
        with pytest.raises(ValueError, match="multinomial model"):
            getattr(multi, name)
    with pytest.raises(NotImplementedError):
        multi.contributions(dense_vc(X))
    with pytest.raises(ValueError, match="unknown LogisticRegression family"):
        LogisticRegression(family="poisson").fit(df)


# ---------------------------------------------------------------------------------------------- 4. pipeline
WORDS = [[f"{name}{i}" for i in range(12)] for name in ("bank", "prize", "parcel")]
COMMON = [f"talk{i}" for i in range(40)]


@functools.lru_cache(maxsize=None)
def dialogues(C=3):
    """A synthetic dialogue frame of ``C`` kinds: common words and a few words of the row's own kind."""
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    rng = np.random.default_rng(41)
    n = 420
    y = rng.integers(0, C, size=n)
    texts = []
    for c in y:
        own = rng.choice(WORDS[c], size=rng.integers(1, 4))
        other = rng.choice(WORDS[(c + 1) % C], size=int(rng.random() < 0.15))
        words = np.concatenate([rng.choice(COMMON, size=rng.integers(8, 30)), own, other])
        texts.append(" ".join(rng.permutation(words)))
    raw = TextColumn(texts)
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.astype(np.float64)})
    return df.take_rows(np.arange(300)), df.take_rows(np.arange(300, n))


@functools.lru_cache(maxsize=None)
def pipeline_model(C=3, family="auto"):
    from fraud_detection_spark_kafka_llm_amd.ml import IDF, HashingTF, LogisticRegression, Pipeline, StopWordsRemover, Tokenizer

    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
              IDF(inputCol="raw_features", outputCol="features"),
              LogisticRegression(featuresCol="features", labelCol="labels", regParam=0.01, maxIter=40, family=family)]
    return Pipeline(stages=stages).fit(dialogues(C)[0])


def staged_outputs(model, df):
    """The staged transform over materialised columns: no fused plan sees the chain."""
    from fraud_detection_spark_kafka_llm_amd.ml import Frame

    cur = df
    for s in model.stages[:-1]:
        cur = s.transform(cur)
    vc = cur.column("features")
    ip, ix, v = vc.csr()
    feats = Frame({"features": VectorColumn(vc.size, ip.clone(), ix.clone(), v.clone()), "labels": df.column("labels")})
    return model.stages[-1].transform(feats), feats.column("features")


def column(frame, name) -> np.ndarray:
    c = frame.column(name)
    return (c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)).astype(np.float64)


def test_pipeline_fused_transform_equals_staged_and_classifies():
    train, test = dialogues()
    model = pipeline_model()
    lrm = model.stages[-1]
    assert lrm.isMultinomial and lrm.numClasses == 3 and lrm.numFeatures == 4096
    for df in (train, test):
        fused = model.transform(df)
        staged, vc = staged_outputs(model, df)
        for name in ("rawPrediction", "probability", "prediction"):
            assert np.array_equal(bits(column(fused, name)), bits(column(staged, name))), name
        raw, prob, pred = (column(fused, n) for n in ("rawPrediction", "probability", "prediction"))
        assert raw.shape == prob.shape == (len(df), 3)
        assert np.array_equal(bits(raw), bits(sparse.score_csr(vc, lrm.class_scorer()).cpu().numpy()))
        assert np.abs(prob.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52
        e = np.exp(raw - raw.max(axis=1, keepdims=True))
        np.testing.assert_allclose(prob, e / e.sum(axis=1, keepdims=True), rtol=8 * 2.0 ** -52)
        assert np.array_equal(pred, np.argmax(prob, axis=1).astype(np.float64))
    y = column(test, "labels")
    acc = float((column(model.transform(test), "prediction") == y).mean())
    print(f"held-out accuracy {acc:.4f} on 3 classes")
    assert acc > 0.9
    sv = staged_outputs(model, test)[1]
    ip, ix, v = (t.cpu().numpy() for t in sv.csr())
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import SparseVector

    one = SparseVector(4096, ix[ip[5]:ip[6]], v[ip[5]:ip[6]])
    staged = staged_outputs(model, test)[0]
    assert np.array_equal(bits(lrm.predictRaw(one).toArray()), bits(column(staged, "rawPrediction")[5]))
    assert np.array_equal(bits(lrm.predictProbability(one).toArray()), bits(column(staged, "probability")[5]))
    assert lrm.predict(one) == column(staged, "prediction")[5]
    with pytest.raises(ValueError, match="3 classes"):
        lrm.scorer()
    with pytest.raises(ValueError, match="3 classes"):
        model.compile(device="cpu")


def test_spark_layout_round_trip_is_bitwise(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LogisticRegressionModel, PipelineModel

    model = pipeline_model()
    path = tmp_path / "mlr_pipeline"
    model.save(str(path))
    assert sf.verify_tree(path) == []
    back = PipelineModel.load(str(path))
    a, b = model.stages[-1], back.stages[-1]
    assert isinstance(b, LogisticRegressionModel) and b.isMultinomial and b.numClasses == 3
    assert np.array_equal(bits(a.coefficientMatrix), bits(b.coefficientMatrix))
    assert np.array_equal(bits(a.interceptVector), bits(b.interceptVector))
    row = sf.read_data_parquet(path / "stages" / f"4_{a.uid}").to_pylist()[0]
    assert row["isMultinomial"] is True and row["numClasses"] == 3 and row["numFeatures"] == 4096
    assert len(row["interceptVector"]["values"]) == 3 and row["coefficientMatrix"]["numRows"] == 3
    assert row["coefficientMatrix"]["type"] == 0 and row["coefficientMatrix"]["isTransposed"]     # mostly zeros: sparse
    test = dialogues()[1]
    for name in ("rawPrediction", "probability", "prediction"):
        assert np.array_equal(bits(column(model.transform(test), name)), bits(column(back.transform(test), name)))
    # a dense matrix (every cell stored, one of them -0.0) takes the dense form and survives as well
    rng = np.random.default_rng(3)
    W = rng.normal(size=(4, 9))
    W[2, 3] = -0.0
    dense = LogisticRegressionModel(coefficientMatrix=W, interceptVector=rng.normal(size=4))
    dense.save(str(tmp_path / "dense"))
    again = LogisticRegressionModel.load(str(tmp_path / "dense"))
    assert sf.read_data_parquet(tmp_path / "dense").to_pylist()[0]["coefficientMatrix"]["type"] == 1
    assert np.array_equal(bits(again.coefficientMatrix), bits(W)) and np.array_equal(bits(again.interceptVector), bits(dense.interceptVector))


def test_a_hand_written_multinomial_model_dir_loads(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LogisticRegressionModel

    W = np.array([[0.5, 0.0, -1.25, 0.0], [0.0, 2.0, 0.0, 0.0], [-0.5, -2.0, 1.25, 3.0]])
    b = np.array([0.1, -0.3, 0.2])
    fields = [sf.Field.simple("numClasses", "integer"), sf.Field.simple("numFeatures", "integer"),
              sf.Field.vector("interceptVector"), sf.Field.matrix("coefficientMatrix"),
              sf.Field.simple("isMultinomial", "boolean")]
    for name, matrix in (("colmajor", sf.dense_matrix(W)), ("sparse", sf.sparse_matrix_row_major(W))):
        d = tmp_path / name
        sf.write_metadata(d, "org.apache.spark.ml.classification.LogisticRegressionModel", "LogisticRegression_abc123",
                          {"regParam": 0.1}, {"family": "auto", "threshold": 0.5})
        sf.write_data_parquet(d, fields, [{"numClasses": 3, "numFeatures": 4, "interceptVector": sf.dense_vector(b),
                                           "coefficientMatrix": matrix, "isMultinomial": True}])
        m = LogisticRegressionModel.load(str(d))
        assert m.isMultinomial and m.numClasses == 3 and m.numFeatures == 4 and m.getRegParam() == 0.1
        assert np.array_equal(bits(m.coefficientMatrix), bits(W)) and np.array_equal(bits(m.interceptVector), bits(b))
        x = np.array([1.0, 0.0, 2.0, 1.0])
        np.testing.assert_allclose(m.predictRaw(x).toArray(), W @ x + b, rtol=1e-15)
        assert m.predict(x) == float(np.argmax(W @ x + b))


def test_binomial_saved_bytes_are_unchanged(tmp_path):
    """The data row of a binomial model is what it was before multinomial models existed."""
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LogisticRegressionModel

    coef = np.array([0.0, 1.5, 0.0, -2.25, 0.0])
    m = LogisticRegressionModel(coef, 0.75)
    m.save(str(tmp_path / "bin"))
    table = sf.read_data_parquet(tmp_path / "bin")
    assert table.schema.names == ["numClasses", "numFeatures", "interceptVector", "coefficientMatrix", "isMultinomial"]
    assert table.to_pylist()[0] == {
        "numClasses": 2, "numFeatures": 5, "interceptVector": sf.dense_vector([0.75]),
        "coefficientMatrix": sf.sparse_matrix_row_major(coef[None, :]), "isMultinomial": False}
    back = LogisticRegressionModel.load(str(tmp_path / "bin"))
    assert not back.isMultinomial and np.array_equal(bits(back.coefficients), bits(coef)) and back.intercept == 0.75
    assert back.numClasses == 2 and back.coefficientMatrix.shape == (1, 5)


@pytest.mark.parametrize("dev", DEVICES)
def test_two_row_model_serves_through_the_single_launch_paths(dev):
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import make_scorer
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    model, test = pipeline_model(2, "multinomial"), dialogues(2)[1]
    lrm = model.stages[-1]
    assert lrm.isMultinomial and lrm.numClasses == 2
    staged, vc = staged_outputs(model, test)
    raw = column(staged, "rawPrediction")
    d = raw[:, 1] - raw[:, 0]
    cs = lrm.class_scorer()
    ip, ix, v = (t.cpu().numpy() for t in vc.csr())
    mag = np.array([np.abs(v[a:e]) @ (np.abs(cs.W[ix[a:e], 0]) + np.abs(cs.W[ix[a:e], 1])) for a, e in zip(ip[:-1], ip[1:])])
    bound = 2 * (np.diff(ip) + 3) * 2.0 ** -53 * (mag + abs(cs.b[0]) + abs(cs.b[1]))
    texts = list(test.column("dialogue").strings)
    fp = model.compile(device=dev)
    pred, prob, rp = (t.cpu().numpy() for t in fp.predict(texts, clean=True))
    m = rp[:, 1]
    assert np.all(rp[:, 0] == 0) and np.all(np.abs(m - d) <= bound)
    sure = np.abs(d) > bound
    assert sure.mean() >= 0.99 and np.array_equal(pred[sure], column(staged, "prediction")[sure])
    np.testing.assert_allclose(prob[:, 1], 1.0 / (1.0 + np.exp(-m)), rtol=4 * 2.0 ** -52)
    sc = make_scorer(fp.spec(True), fp.idf.idf, lrm.scorer(), dev, max_docs=256, max_bytes=256 * 4096)
    ring = PinnedRing(slots=1, max_docs=256, max_bytes=256 * 4096)
    ring.slots[0].fill(texts)
    sm = sc.score_packed(ring.slots[0])
    assert np.array_equal(bits(sm[:, 0]), bits(m))
    spred, sp1 = lrm.postprocess_numpy(np.array(sm))
    assert np.array_equal(spred, pred)
    np.testing.assert_allclose(sp1, prob[:, 1], rtol=4 * 2.0 ** -52)


def test_train_cli_fits_a_multinomial_model_on_request(tmp_path):
    from fraud_detection_spark_kafka_llm_amd import train

    common = ["--data", "", "--synthetic", "300", "--no-plots", "--num-trees", "2", "--max-depth", "2",
              "--out-dir", str(tmp_path), "--device", "cpu"]
    summary = train.main(common + ["--lr-label-col", "labels"])
    assert summary["MultinomialLogisticRegression"]["Test"]["Accuracy"] > 0.9
    assert summary["MultinomialLogisticRegression"]["numClasses"] == 2
    with pytest.raises(ValueError, match="not integer-coded"):
        train.integer_codes(dialogues()[0], "dialogue")


# ---------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("dev", DEVICES)
def test_two_fits_are_bitwise_equal(dev):
    X, y = opt_corpus(4)
    w = np.random.default_rng(1).choice([0.5, 3.0], size=len(y))
    fits = [LR.train_multinomial_logistic_regression(dense_vc(X, dev), y, weights=w, reg_param=0.01, max_iter=30, device=dev)
            for _ in range(2)]
    assert fits[0][0].tobytes() == fits[1][0].tobytes() and fits[0][1].tobytes() == fits[1][1].tobytes()
    assert fits[0][2] == fits[1][2]


def _dp_fit(rank, world, std):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = opt_corpus(3)
    lo, hi = shard_range(len(y), rank, world)
    W, b, h = LR.train_multinomial_logistic_regression(dense_vc(X[lo:hi]), y[lo:hi], reg_param=0.01, standardization=std,
                                                       max_iter=30, device="cpu")
    return W.tobytes(), b.tobytes(), h


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_fit_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    X, y = opt_corpus(3)
    single = LR.train_multinomial_logistic_regression(dense_vc(X), y, reg_param=0.01, standardization=False, max_iter=30,
                                                      device="cpu")
    outs = spawn(_dp_fit, world, False, backend="gloo")
    assert all(o == outs[0] for o in outs)
    assert outs[0] == (single[0].tobytes(), single[1].tobytes(), single[2])                  # bitwise
    single = LR.train_multinomial_logistic_regression(dense_vc(X), y, reg_param=0.01, standardization=True, max_iter=30,
                                                      device="cpu")
    outs = spawn(_dp_fit, world, True, backend="gloo")
    np.testing.assert_allclose(np.frombuffer(outs[0][0]).reshape(3, -1), single[0], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(np.frombuffer(outs[0][1]), single[1], rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------------------------------------- 6. self-test
def test_mlr_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--mlr-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "mlr selftest ok" in res.stdout
