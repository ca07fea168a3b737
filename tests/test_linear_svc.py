"""Linear SVC (csrc/svc.h, svc_kernels.hip, svc_cpu.cpp, ops.sparse.svc_eval, models/svm.py, ml.LinearSVC and
its model): the fused exact hinge pass against an integer oracle written here, the trainer against
scikit-learn's dual coordinate descent, and the Spark surface (params, persistence, serving).

The contract (README "Linear SVC"): ``m_i = b + sum_j val[j] xs[idx[j]]`` in ``spmv``'s order (lane ``l`` of 64
adds the entries ``l, l + 64, ...`` ascending, multiply then add; the xor butterfly over 32 .. 1; then ``+ b``),
``s = 2 y - 1``, ``z = 1 - s m``, ``loss = z < 2048 ? max(z, 0) : 2048``, ``r = z > 0 ? - s w : 0``, and the
int64 sums ``Gq[f] = sum rint((x r) 2^k)``, ``gbq = sum rint(r 2^k)``, ``lossq = sum rint((w loss) 2^kl)``,
``nact = #{r != 0}``. Every term is exactly rounded fp64 arithmetic, so the whole block is the same bits on
the host, on the device and for every grid, hot set, chunk size, thread count and world size.
"""
import functools
import json
import math
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.models import svm as SVM
from fraud_detection_spark_kafka_llm_amd.ops import sparse

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
F = 300
LIM = sparse.svc_limits()
CHUNK = LIM["chunk_rows"]
EDGE_LENS = [200, 65, 0, 64, 1, 63]      # the first rows of every corpus (a corpus of n < 6 rows holds a prefix)
CLAMPED, BAD = int(LIM["flag_clamped"]), int(LIM["flag_bad_input"])


def bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------- 1. the pass
@functools.lru_cache(maxsize=None)
def corpus(n, dtype_name="float64", weighted=False, size=F, seed=5, max_feature=None):
    """CSR (numpy), labels, weights or None, xs, b. Margins have a standard deviation near 2, so rows
    inside and outside the margin mix; values are negative now and then."""
    rng = np.random.default_rng(seed + n)
    lens = (EDGE_LENS + list(rng.integers(0, 41, size=max(n - len(EDGE_LENS), 0))))[:n]
    hi = max_feature or size
    idx = np.concatenate([rng.choice(hi, size=k, replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = (rng.choice([-1.0, 1.0], p=[0.15, 0.85], size=idx.size) * (0.1 + 2.9 * rng.random(idx.size))).astype(dtype_name)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    y = rng.integers(0, 2, size=n).astype(np.float64)
    w = rng.choice([0.0, 0.5, 3.0], p=[0.1, 0.45, 0.45], size=n) if weighted else None
    xs = 0.8 * rng.random(size) - 0.4
    return (indptr, idx, val), y, w, xs, float(rng.random() - 0.5)


def exponents(csr, w, n):
    return sparse.mlr_scale_exponents(1.0 if w is None else max(float(w.max()), 0.0),
                                      float(np.abs(csr[2]).max()) if csr[2].size else 0.0, n)


def run_eval(csr, y, w, xs, b, dev, k=None, kl=None, hot=None, **kw):
    """``svc_eval`` on ``dev``; ``hot`` is a list of feature ids (device only) or None for no hot set."""
    n = csr[0].size - 1
    if k is None:
        k, kl = exponents(csr, w, n)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in csr]
    tables = (None, None)
    if hot is not None and torch.device(dev).type == "cuda":
        tables = sparse.nb_hot_tables(torch.as_tensor(hot, dtype=torch.int32, device=dev), xs.size, 1)
    return sparse.svc_eval(t[0], t[1], t[2], torch.from_numpy(xs).to(dev), b, torch.from_numpy(y).to(dev),
                           None if w is None else torch.from_numpy(w).to(dev), k, kl, tables, **kw)


def oracle_margin(csr, xs, b, r) -> float:
    """``spmv``'s order in Python floats (fp64, one rounding per operation)."""
    indptr, idx, val = csr
    p = [0.0] * 64
    for j in range(indptr[r], indptr[r + 1]):
        p[(j - indptr[r]) % 64] += float(val[j]) * float(xs[idx[j]])
    o = 32
    while o:
        for lane in range(o):
            p[lane] = p[lane] + p[lane + o]
        o //= 2
    return p[0] + b


def quant(t: float, k: int) -> int:
    return round(Fraction(t) * 2 ** k)           # exact scaling, ties to even


def integer_oracle(csr, y, w, xs, b, k, kl):
    """The block by the contract in Python integers, and the per-row (margin, r, loss)."""
    indptr, idx, val = csr
    size = xs.size
    out = [0] * (size + 4)
    rows = []
    for r in range(indptr.size - 1):
        m = oracle_margin(csr, xs, b, r)
        wr = 1.0 if w is None else float(w[r])
        s = 2.0 * float(y[r]) - 1.0
        z = 1.0 - s * m
        clamped = not (z < 2048.0)
        loss = 2048.0 if clamped else (z if z > 0.0 else 0.0)
        res = -s * wr if z > 0.0 else 0.0
        rows.append((m, res, loss))
        if clamped:
            out[size + 3] |= CLAMPED
        out[size + 1] += quant(wr * loss, kl)
        if res == 0.0:
            continue
        out[size] += quant(res, k)
        out[size + 2] += 1
        for j in range(indptr[r], indptr[r + 1]):
            out[idx[j]] += quant(float(val[j]) * res, k)
    return np.array(out, dtype=np.int64), np.array(rows, dtype=np.float64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def oracle_of(n, dtype_name, weighted):
    csr, y, w, xs, b = corpus(n, dtype_name, weighted)
    return integer_oracle(csr, y, w, xs, b, *exponents(csr, w, n))


def host_block(n, dtype_name, weighted) -> np.ndarray:
    return run_eval(*corpus(n, dtype_name, weighted), "cpu").block.numpy()


def test_limits_are_exported():
    assert LIM["hot_slots"] == 4096 and LIM["max_hot_slots"] == 8064 and LIM["loss_cap"] == 2048.0
    assert LIM["table_bytes"] == 32 * 1024 and LIM["max_table_bytes"] == 63 * 1024 and CHUNK == 1024


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("n", [3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_block_equals_the_integer_oracle(n, dtype_name, weighted, dev):
    csr, y, w, xs, b = corpus(n, dtype_name, weighted)
    want, rows = oracle_of(n, dtype_name, weighted)
    got = run_eval(csr, y, w, xs, b, dev, want_rows=True)
    block = got.block.cpu().numpy()
    assert np.array_equal(block[:F], want[:F]), "Gq"
    assert (got.gbq, got.lossq, got.nact, got.flag) == tuple(int(v) for v in want[F:])
    assert np.array_equal(got.Gq.cpu().numpy(), want[:F]) and not got.clamped and not got.bad_input
    # the device block is the host block bit for bit, lossq included
    assert np.array_equal(block, host_block(n, dtype_name, weighted))
    for col, t in enumerate((got.margin, got.r, got.loss_row)):
        assert np.array_equal(bits(t), bits(rows[:, col])), ("margin", "r", "loss_row")[col]
    if n > 6:
        assert 0 < got.nact < n                    # rows inside and outside the margin
    # the margin is spmv + b bit for bit
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in csr]
    assert np.array_equal(bits(sparse.spmv(t[0], t[1], t[2], torch.from_numpy(xs).to(dev)) + b), bits(got.margin))


# ---------------------------------------------------------------------------------------------- 2. hinge edges
def rows_csr(rows, dtype=np.float64):
    """CSR of a list of rows, each a list of (feature, value)."""
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    idx = np.array([f for r in rows for f, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=dtype)
    return indptr, idx, val


@pytest.mark.parametrize("dev", DEVICES)
def test_a_row_exactly_on_the_margin_is_inactive(dev):
    # dyadic values: m = 0.75 + 0.25 = 1 and m = -1.25 + 0.25 = -1 exactly
    xs = np.zeros(8)
    xs[0], xs[1], xs[2] = 0.75, -1.25, 0.5
    csr = rows_csr([[(0, 1.0)], [(0, 1.0)], [(1, 1.0)], [(1, 1.0)], [(2, 1.0)]])
    y = np.array([1.0, 0.0, 0.0, 1.0, 1.0])
    got = run_eval(csr, y, None, xs, 0.25, dev, k=20, kl=20, want_rows=True)
    assert got.margin.tolist() == [1.0, 1.0, -1.0, -1.0, 0.75]
    assert got.r.tolist() == [0.0, 1.0, 0.0, -1.0, -1.0]           # s m == 1 exactly: inactive
    assert got.loss_row.tolist() == [0.0, 2.0, 0.0, 2.0, 0.25]
    assert got.nact == 3 and got.gbq == -(1 << 20) and got.lossq == int(4.25 * 2 ** 20) and got.flag == 0
    assert got.Gq.tolist() == [1 << 20, -(1 << 20), -(1 << 20), 0, 0, 0, 0, 0]


@pytest.mark.parametrize("dev", DEVICES)
def test_all_inactive_and_all_active_corpora(dev):
    n = CHUNK + 3
    csr, _, _, xs, _ = corpus(n)
    # every row on its own side, far from the margin: labels follow the margin, which is scaled up
    m = np.array([oracle_margin(csr, xs, 0.0, r) for r in range(n)])
    far = np.abs(m) > 1e-3
    y = (m > 0).astype(np.float64)
    w = far.astype(np.float64)                                       # the few rows near 0 (empty rows): weight 0
    got = run_eval(csr, y, w, xs * 1024.0, 0.0, dev)                 # |m| > 1.024: s m > 1
    assert torch.count_nonzero(got.Gq) == 0 and got.gbq == 0 and got.nact == 0 and got.lossq == 0 and got.flag == 0
    # beta = 0, b = 0: every row is active with loss 1
    k, kl = exponents(csr, None, n)
    y = corpus(n)[1]
    got = run_eval(csr, y, None, np.zeros(F), 0.0, dev, k=k, kl=kl)
    assert got.nact == n and got.lossq == n << kl and got.gbq == int((n - 2 * y.sum())) << k and got.flag == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_zero_weight_rows_add_nothing_and_are_not_counted(dev):
    n = CHUNK + 3
    csr, y, w, xs, b = corpus(n, weighted=True)
    k, kl = exponents(csr, w, n)
    zero = w == 0
    assert 0 < zero.sum() < n
    keep = np.flatnonzero(~zero)
    indptr, idx, val = csr
    sub = rows_csr([list(zip(idx[indptr[r]:indptr[r + 1]], val[indptr[r]:indptr[r + 1]])) for r in keep])
    a = run_eval(csr, y, w, xs, b, dev, k=k, kl=kl, want_rows=True)
    c = run_eval(sub, y[keep], w[keep], xs, b, dev, k=k, kl=kl)
    assert torch.equal(a.block, c.block)
    assert not a.r[torch.from_numpy(zero).to(dev)].any() and a.nact <= keep.size


@pytest.mark.parametrize("dev", DEVICES)
def test_a_margin_of_5000_against_the_label_is_clamped_and_flagged(dev):
    xs = np.array([5000.0, 0.25])
    csr = rows_csr([[(0, 1.0)], [(1, 1.0)], [(0, 1.0)]])
    y = np.array([0.0, 1.0, 1.0])
    got = run_eval(csr, y, np.array([3.0, 1.0, 1.0]), xs, 0.0, dev, k=10, kl=10, want_rows=True)
    assert got.flag == CLAMPED and got.clamped and not got.bad_input
    assert got.loss_row.tolist() == [2048.0, 0.75, 0.0] and got.r.tolist() == [3.0, -1.0, 0.0]
    assert got.lossq == int((3 * 2048 + 0.75) * 2 ** 10) and got.nact == 2
    assert got.Gq.tolist() == [3 << 10, -(1 << 10)]
    # a NaN coefficient: the row is clamped and has no residual
    got = run_eval(csr, y, None, np.array([math.nan, 0.25]), 0.0, dev, k=10, kl=10, want_rows=True)
    assert got.flag == CLAMPED and got.r.tolist() == [0.0, -1.0, 0.0] and got.loss_row.tolist() == [2048.0, 0.75, 2048.0]
    assert got.Gq.tolist() == [0, -(1 << 10)] and got.nact == 1


# ---------------------------------------------------------------------------------------------- 3. speed knobs
@pytest.mark.parametrize("dev", DEVICES)
def test_hot_set_chunk_and_threads_change_no_bit(dev):
    size, n = 10_000, 2 * CHUNK + 1                                  # more features than the largest table holds
    csr, y, w, xs, b = corpus(n, "float32", True, size=size, max_feature=size - 50)
    ref = run_eval(csr, y, w, xs, b, "cpu", threads=1).block
    assert torch.count_nonzero(ref[:size]) > LIM["max_hot_slots"] // 2
    df = np.bincount(csr[1], minlength=size)
    by_freq = np.argsort(-df, kind="stable")
    hots = {"none": None, "one": by_freq[:1], "default": by_freq[:LIM["hot_slots"]], "largest": by_freq[:LIM["max_hot_slots"]],
            "absent": np.arange(size - 100, size), "rare": by_freq[::-1][:LIM["hot_slots"]]}
    assert LIM["max_hot_slots"] < (df > 0).sum()                     # cold and hot entries mix
    for name, hot in hots.items():
        got = run_eval(csr, y, w, xs, b, dev, hot=None if hot is None else list(hot))
        assert torch.equal(got.block.cpu(), ref), name
    for chunk in (1, 7, 1024):
        got = run_eval(csr, y, w, xs, b, dev, hot=list(hots["default"]), chunk_rows=chunk)
        assert torch.equal(got.block.cpu(), ref), chunk
    for threads in (1, 3):
        assert torch.equal(run_eval(csr, y, w, xs, b, dev, threads=threads).block.cpu(), ref), threads
    with pytest.raises(ValueError, match="exceeds the LDS table"):
        sparse.nb_hot_tables(torch.arange(LIM["max_hot_slots"] + 1, dtype=torch.int32), size, 1)


def test_argument_errors_raise_before_any_launch():
    csr, y, w, xs, b = corpus(5)
    t = [torch.from_numpy(a) for a in csr]
    ok = dict(xs=torch.from_numpy(xs), b=b, y=torch.from_numpy(y), w=None, k=20, kl=20)
    for change in (dict(k=-1), dict(kl=LIM["k_max"] + 1), dict(xs=torch.zeros(F, dtype=torch.float32)),
                   dict(xs=torch.zeros((F, 1), dtype=torch.float64)), dict(y=torch.zeros(4, dtype=torch.float64)),
                   dict(w=torch.ones(6, dtype=torch.float64)), dict(chunk_rows=-1)):
        with pytest.raises(ValueError, match="svc_eval"):
            sparse.svc_eval(t[0], t[1], t[2], **{**ok, **change})
    with pytest.raises(ValueError, match="svc_eval"):
        sparse.svc_eval(t[0], t[1].to(torch.int64), t[2], **ok)
    with pytest.raises(ValueError, match="within idx"):
        sparse.svc_eval(t[0] + 1, t[1], t[2], **ok)


# ---------------------------------------------------------------------------------------------- 4. bad input
BAD_CASES = [("label", 0.5), ("label", 2.0), ("label", -1.0), ("label", math.nan), ("weight", -1.0), ("weight", math.nan),
             ("weight", math.inf), ("value", math.nan), ("value", math.inf), ("value", -math.inf), ("feature", -1),
             ("feature", F)]


@pytest.mark.parametrize("dev", DEVICES)
def test_bad_input_sets_the_high_flag_half_and_adds_nothing(dev):
    n = CHUNK + 3
    csr, y, w, xs, b = corpus(n, weighted=True)
    k, kl = exponents(csr, w, n)
    row = 1                                                          # 65 entries
    gone = w.copy()
    gone[row] = 0.0
    want = run_eval(csr, y, gone, xs, b, "cpu", k=k, kl=kl).block.clone()
    want[-1] = BAD
    at = int(csr[0][row]) + 64
    for kind, bad in BAD_CASES:
        indptr, idx, val = (a.copy() for a in csr)
        y2, w2 = y.copy(), w.copy()
        w2[row] = 3.0
        if kind == "label":
            y2[row] = bad
        elif kind == "weight":
            w2[row] = bad
        elif kind == "value":
            val[at] = bad
        else:
            idx[at] = bad
        got = run_eval((indptr, idx, val), y2, w2, xs, b, dev, k=k, kl=kl, want_rows=True)
        assert torch.equal(got.block.cpu(), want), (kind, bad)
        assert got.bad_input and not got.clamped and float(got.r[row]) == 0.0 and float(got.loss_row[row]) == 0.0


def dense_vc(X, dev="cpu") -> VectorColumn:
    return VectorColumn(X.shape[1], dense=torch.from_numpy(np.array(X, dtype=np.float64)).to(dev))


@pytest.mark.parametrize("dev", DEVICES)
def test_trainer_and_estimator_raise_before_any_model(dev):
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, LinearSVC

    rng = np.random.default_rng(0)
    X = rng.normal(size=(40, 6)) * (rng.random((40, 6)) < 0.5)
    y = (rng.random(40) < 0.5).astype(np.float64)
    fit = functools.partial(SVM.train_linear_svc, device=dev, max_iter=3)
    for bad in (2.0, 0.5, -1.0, math.nan):
        y2 = y.copy()
        y2[7] = bad
        with pytest.raises(ValueError, match="labels must be 0 or 1"):
            fit(dense_vc(X), y2)
        with pytest.raises(ValueError, match="labels must be 0 or 1"):
            LinearSVC(labelCol="y").fit(Frame({"features": dense_vc(X), "y": y2}))
    for bad in (-0.5, math.nan, math.inf):
        w = np.ones(40)
        w[3] = bad
        with pytest.raises(ValueError, match="weights must be finite and >= 0"):
            fit(dense_vc(X), y, weights=w)
        with pytest.raises(ValueError, match="weights must be finite and >= 0"):
            LinearSVC(labelCol="y", weightCol="w").fit(Frame({"features": dense_vc(X), "y": y, "w": w}))
    for bad in (math.nan, math.inf):
        X2 = X.copy()
        X2[np.nonzero(X2)[0][0], np.nonzero(X2)[1][0]] = bad
        with pytest.raises(ValueError, match="finite feature values"):
            fit(dense_vc(X2), y)
    with pytest.raises(ValueError, match="positive weight sum"):
        fit(dense_vc(X), y, weights=np.zeros(40))
    with pytest.raises(ValueError, match="one entry per row"):
        fit(dense_vc(X), y[:-1])
    with pytest.raises(ValueError, match="one entry per row"):
        fit(dense_vc(X), y, weights=np.ones(41))
    with pytest.raises(ValueError, match="reg_param"):
        fit(dense_vc(X), y, reg_param=-0.1)


# ---------------------------------------------------------------------------------------------- 5. the optimum
# Relative gap of the fitted objective above scikit-learn's dual coordinate descent (run to tol 1e-10),
# both evaluated by `objective` below. Measured on the host over the cases of this file (figures in
# profiles/r18/linear_svc.md): over OPT_CASES the gaps are 3.4e-6 .. 3.23e-3 (the worst at 300 x 40,
# regParam 0.001, where L-BFGS on the subgradient stops after 50 iterations), over STD_CASES 1.10e-3 and
# 3.90e-3. Each bound is its worst gap times 3 for other seeds and the device's different dot-product order.
OPT_GAP_BOUND = 3 * 3.23e-3
STD_GAP_BOUND = 3 * 3.90e-3
OPT_CASES = [(n, f, reg) for n, f in ((300, 40), (2000, 200)) for reg in (0.1, 0.01, 0.001)]
STD_CASES = [(300, 40, 0.01), (2000, 200, 0.01)]


@functools.lru_cache(maxsize=None)
def opt_corpus(n, f):
    rng = np.random.default_rng(17 + n)
    X = rng.normal(size=(n, f)) * (rng.random((n, f)) < 0.05)
    truth = rng.normal(size=f)
    y = (X @ truth + 0.3 * rng.normal(size=n) + 0.2 > 0).astype(np.float64)
    return X, y


def objective(X, y, beta, b, reg) -> float:
    return float(np.maximum(0.0, 1.0 - (2.0 * y - 1.0) * (X @ beta + b)).mean() + 0.5 * reg * beta @ beta)


def sample_std(X) -> np.ndarray:
    return X.std(axis=0, ddof=1)


@functools.lru_cache(maxsize=None)
def reference(n, f, reg, std):
    """scikit-learn's model: raw features and no intercept, or columns scaled to unit sample variance
    and an intercept that is all but unpenalised (``intercept_scaling`` = 30: its share of the penalty is below 1e-5 of the objective)."""
    from sklearn.svm import LinearSVC

    X, y = opt_corpus(n, f)
    if std:
        X = X / sample_std(X)
    sk = LinearSVC(loss="hinge", dual=True, C=1.0 / (n * reg), fit_intercept=std, intercept_scaling=30.0, tol=1e-10,
                   max_iter=2_000_000).fit(X, y)
    return sk.coef_[0].copy(), float(sk.intercept_[0]) if std else 0.0


@functools.lru_cache(maxsize=None)
def fitted(n, f, reg, std, dev):
    X, y = opt_corpus(n, f)
    return SVM.train_linear_svc(dense_vc(X, dev), y, reg_param=reg, fit_intercept=std, standardization=std, device=dev)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n,f,reg", OPT_CASES)
def test_fit_reaches_sklearns_optimum_on_raw_features(n, f, reg, dev):
    X, y = opt_corpus(n, f)
    coef, intercept, history = fitted(n, f, reg, False, dev)
    ref_coef, _ = reference(n, f, reg, False)
    ours, ref = objective(X, y, coef, 0.0, reg), objective(X, y, ref_coef, 0.0, reg)
    agree = float(((X @ coef > 0) == (X @ ref_coef > 0)).mean())
    print(f"{n}x{f} regParam {reg}: objective {ours:.9f} sklearn {ref:.9f} gap {(ours - ref) / ref:.3e} "
          f"equal predictions {agree:.4f} iterations {len(history) - 1}")
    assert intercept == 0.0 and (ours - ref) / ref <= OPT_GAP_BOUND
    assert history[-1] == pytest.approx(ours, rel=1e-9)
    assert all(a >= b for a, b in zip(history, history[1:])) and history[0] == 1.0 and history[-1] < 1.0


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n,f,reg", STD_CASES)
def test_fit_with_intercept_and_standardization_reaches_sklearns_optimum(n, f, reg, dev):
    X, y = opt_corpus(n, f)
    sd = sample_std(X)
    assert sd.min() > 0
    coef, intercept, history = fitted(n, f, reg, True, dev)
    ref_coef, ref_b = reference(n, f, reg, True)
    Xs = X / sd
    # the penalty is on the coefficients of the scaled columns: coef = beta / std
    ours, ref = objective(Xs, y, coef * sd, intercept, reg), objective(Xs, y, ref_coef, ref_b, reg)
    print(f"{n}x{f} regParam {reg} standardized: objective {ours:.9f} sklearn {ref:.9f} gap {(ours - ref) / ref:.3e}")
    assert (ours - ref) / ref <= STD_GAP_BOUND and intercept != 0.0
    assert history[-1] == pytest.approx(ours, rel=1e-9)
    assert all(a >= b for a, b in zip(history, history[1:])) and history[-1] < history[0] == 1.0


# ---------------------------------------------------------------------------------------------- 6. device ~ host
@pytest.mark.gpu
@pytest.mark.parametrize("n,f,reg,std", [(300, 40, 0.01, False), (2000, 200, 0.001, False), (2000, 200, 0.01, True)])
def test_device_fit_reaches_the_host_fits_objective(n, f, reg, std):
    X, y = opt_corpus(n, f)
    Xs = X / sample_std(X) if std else X
    sd = sample_std(X) if std else 1.0
    host, dev = fitted(n, f, reg, std, "cpu"), fitted(n, f, reg, std, "cuda:0")
    a, b = objective(Xs, y, host[0] * sd, host[1], reg), objective(Xs, y, dev[0] * sd, dev[1], reg)
    print(f"{n}x{f} regParam {reg}: host {a:.9f} device {b:.9f}")
    assert abs(a - b) / a <= (STD_GAP_BOUND if std else OPT_GAP_BOUND)


@pytest.mark.parametrize("dev", DEVICES)
def test_two_fits_are_bitwise_equal(dev):
    X, y = opt_corpus(300, 40)
    w = np.random.default_rng(1).choice([0.5, 3.0], size=len(y))
    fits = [SVM.train_linear_svc(dense_vc(X, dev), y, weights=w, reg_param=0.01, max_iter=30, device=dev) for _ in range(2)]
    assert fits[0][0].tobytes() == fits[1][0].tobytes() and fits[0][1] == fits[1][1] and fits[0][2] == fits[1][2]
    assert SVM.SVC_STATS["iterations"] == len(fits[1][2]) - 1 and 0 < SVM.SVC_STATS["active_share"] <= 1


@pytest.mark.parametrize("dev", DEVICES)
def test_a_clamped_trial_is_rejected_like_an_infinite_objective(dev, monkeypatch):
    X, y = opt_corpus(300, 40)
    seen = []
    real = SVM._lbfgs

    def spy(fg, theta, *a, first=False):
        far = theta.clone()
        far[0] = 1e6                                                  # margins of 1e6 on the rows that hold feature 0
        if not first:
            fg(theta)
        seen.append(fg(far)[0])
        return real(fg, theta, *a)

    monkeypatch.setattr(SVM, "_lbfgs", spy)
    fit = functools.partial(SVM.train_linear_svc, reg_param=0.01, standardization=False, max_iter=5, device=dev)
    coef, _, history = fit(dense_vc(X, dev), y)
    assert seen == [math.inf] and all(math.isfinite(h) for h in history) and np.isfinite(coef).all()
    # a clamped first evaluation has nothing to fall back to
    monkeypatch.setattr(SVM, "_lbfgs", functools.partial(spy, first=True))
    with pytest.raises(ValueError, match="starting point"):
        fit(dense_vc(X, dev), y)


# ---------------------------------------------------------------------------------------------- 7. data parallel
def _dp_fit(rank, world, std):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = opt_corpus(300, 40)
    lo, hi = shard_range(len(y), rank, world)
    coef, b, h = SVM.train_linear_svc(dense_vc(X[lo:hi]), y[lo:hi], reg_param=0.01, standardization=std, max_iter=30,
                                      device="cpu")
    return coef.tobytes(), b, h


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_fit_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    X, y = opt_corpus(300, 40)
    single = SVM.train_linear_svc(dense_vc(X), y, reg_param=0.01, standardization=False, max_iter=30, device="cpu")
    outs = spawn(_dp_fit, world, False, backend="gloo")
    assert all(o == outs[0] for o in outs)
    assert outs[0] == (single[0].tobytes(), single[1], single[2])                            # bitwise
    single = SVM.train_linear_svc(dense_vc(X), y, reg_param=0.01, standardization=True, max_iter=30, device="cpu")
    outs = spawn(_dp_fit, world, True, backend="gloo")
    np.testing.assert_allclose(np.frombuffer(outs[0][0]), single[0], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(outs[0][1], single[1], rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------------------------------------- 8. API
def test_params_defaults_and_order():
    from fraud_detection_spark_kafka_llm_amd.ml import LinearSVC, LinearSVCModel

    want = {"featuresCol": "features", "labelCol": "label", "predictionCol": "prediction", "rawPredictionCol": "rawPrediction",
            "maxIter": 100, "regParam": 0.0, "tol": 1e-6, "fitIntercept": True, "standardization": True, "threshold": 0.0,
            "aggregationDepth": 2, "maxBlockSizeInMB": 0.0}
    for obj in (LinearSVC(), LinearSVCModel([1.0, -2.0], 0.5)):
        assert obj._defaultParamMap == want and list(obj._defaultParamMap) == list(want)
        names = [p.name for p in obj.params()]
        assert "probabilityCol" not in names and "weightCol" in names and not obj.isDefined("weightCol")
        with pytest.raises(AttributeError):
            obj.getProbabilityCol()
        assert obj.uid.startswith("LinearSVC_")
    assert LinearSVC._java_class == "org.apache.spark.ml.classification.LinearSVC"
    assert LinearSVCModel._java_class == "org.apache.spark.ml.classification.LinearSVCModel"
    with pytest.raises(AttributeError):
        LinearSVC(probabilityCol="p")


def test_model_surface_and_threshold():
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, LinearSVC
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import SparseVector

    X, y = opt_corpus(300, 40)
    frame = Frame({"features": dense_vc(X), "label": y})
    model = LinearSVC(regParam=0.01, maxIter=30).fit(frame)
    assert model.numClasses == 2 and model.numFeatures == 40 and model.coefficients.shape == (40,)
    assert len(model.objectiveHistory) > 1 and model.getRegParam() == 0.01 and model.getThreshold() == 0.0
    out = model.transform(frame)
    assert "probability" not in out.columns and {"rawPrediction", "prediction"} <= set(out.columns)
    raw, pred = out.column("rawPrediction").numpy(), out.column("prediction").numpy()
    m = raw[:, 1]
    np.testing.assert_allclose(m, X @ model.coefficients + model.intercept, rtol=0, atol=1e-12)
    assert np.array_equal(bits(raw[:, 0]), bits(-m)) and np.array_equal(pred, (m > 0).astype(np.float64))
    assert float((pred == y).mean()) > 0.85
    moved = model.copy({"threshold": 0.5}).transform(frame)
    assert np.array_equal(bits(moved.column("rawPrediction")), bits(raw))
    assert np.array_equal(moved.column("prediction").numpy(), (m > 0.5).astype(np.float64))
    assert 0 < (moved.column("prediction").numpy() != pred).sum()
    for i in (0, 5, 17):
        nz = np.flatnonzero(X[i])
        one = SparseVector(40, nz, X[i, nz])
        assert np.array_equal(bits(model.predictRaw(one).toArray()), bits(raw[i])) and model.predict(one) == pred[i]
    # the serving triple: a monotone squashing of the margin around the threshold, > 0.5 iff the prediction is 1
    rp, conf, p = model.copy({"threshold": 0.5}).postprocess(torch.from_numpy(m.copy()).reshape(-1, 1))
    np.testing.assert_allclose(conf[:, 1].numpy(), 1.0 / (1.0 + np.exp(-(m - 0.5))), rtol=4 * 2.0 ** -52)
    assert np.array_equal((conf[:, 1] > 0.5).numpy(), p.numpy() == 1.0) and np.array_equal(bits(rp), bits(raw))
    # contributions: a row sums to the margin
    c = model.contributions(frame)
    ip, ix, v = (t.numpy() for t in c.csr())
    assert c.size == 41
    np.testing.assert_allclose(np.add.reduceat(v, ip[:-1]), m, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- 9. persistence
def test_spark_layout_round_trip_is_bitwise(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LinearSVC, LinearSVCModel

    rng = np.random.default_rng(3)
    coef = rng.normal(size=9)
    coef[4] = -0.0
    m = LinearSVCModel(coef, -0.375, regParam=0.25, threshold=0.125, weightCol="w")
    path = tmp_path / "svc"
    m.save(str(path))
    assert sf.verify_tree(path) == [] and (path / "data" / "_SUCCESS").exists() and (path / "metadata" / "_SUCCESS").exists()
    assert any(p.name.endswith(".crc") for p in (path / "data").iterdir())
    md = sf.read_metadata(path)
    assert md["class"] == "org.apache.spark.ml.classification.LinearSVCModel" and md["uid"] == m.uid
    assert md["paramMap"] == {"regParam": 0.25, "threshold": 0.125, "weightCol": "w"}
    assert list(md["defaultParamMap"]) == list(m._defaultParamMap) and "probabilityCol" not in md["defaultParamMap"]
    table = sf.read_data_parquet(path)
    assert table.schema.names == ["coefficients", "intercept"] and table.num_rows == 1
    assert table.to_pylist()[0] == {"coefficients": sf.dense_vector(coef), "intercept": -0.375}
    back = LinearSVCModel.load(str(path))
    assert np.array_equal(bits(back.coefficients), bits(coef)) and back.intercept == -0.375
    assert back._paramMap == m._paramMap and back._defaultParamMap == m._defaultParamMap and back.uid == m.uid
    est = LinearSVC(maxIter=7, regParam=0.5)
    est.save(str(tmp_path / "est"))
    again = LinearSVC.load(str(tmp_path / "est"))
    assert sf.read_metadata(tmp_path / "est")["class"] == "org.apache.spark.ml.classification.LinearSVC"
    assert again.getMaxIter() == 7 and again.getRegParam() == 0.5 and again._defaultParamMap == est._defaultParamMap


def test_a_hand_written_model_dir_loads(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LinearSVCModel
    from fraud_detection_spark_kafka_llm_amd.ml.base import Params

    coef = np.array([0.5, 0.0, -1.25, 3.0])
    for name, vec in (("dense", sf.dense_vector(coef)), ("sparse", sf.sparse_vector(4, [0, 2, 3], [0.5, -1.25, 3.0]))):
        d = tmp_path / name
        sf.write_metadata(d, "org.apache.spark.ml.classification.LinearSVCModel", "LinearSVC_abc123",
                          {"regParam": 0.1, "threshold": 0.25}, {"maxIter": 100, "threshold": 0.0, "tol": 1e-6})
        sf.write_data_parquet(d, [sf.Field.vector("coefficients"), sf.Field.simple("intercept", "double")],
                              [{"coefficients": vec, "intercept": -0.75}])
        m = Params.load(str(d))
        assert isinstance(m, LinearSVCModel) and m.uid == "LinearSVC_abc123" and m.numFeatures == 4
        assert np.array_equal(bits(m.coefficients), bits(coef)) and m.intercept == -0.75
        assert m.getRegParam() == 0.1 and m.getThreshold() == 0.25 and m.getMaxIter() == 100
        x = np.array([1.0, 5.0, 2.0, 0.5])
        assert m.predictRaw(x).toArray().tolist() == [1.25, -1.25] and m.predict(x) == 0.0
        assert m.copy({"threshold": -2.0}).predict(x) == 1.0


def test_binomial_logistic_regression_saved_bytes_are_unchanged(tmp_path):
    """A binomial LogisticRegressionModel saved next to a LinearSVCModel is what it was before."""
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LinearSVCModel, LogisticRegressionModel

    coef = np.array([0.0, 1.5, 0.0, -2.25, 0.0])
    LinearSVCModel(coef, 0.75).save(str(tmp_path / "svc"))
    m = LogisticRegressionModel(coef, 0.75, uid="LogisticRegression_0123456789ab")
    m.save(str(tmp_path / "bin"))
    table = sf.read_data_parquet(tmp_path / "bin")
    assert table.schema.names == ["numClasses", "numFeatures", "interceptVector", "coefficientMatrix", "isMultinomial"]
    assert table.to_pylist()[0] == {
        "numClasses": 2, "numFeatures": 5, "interceptVector": sf.dense_vector([0.75]),
        "coefficientMatrix": sf.sparse_matrix_row_major(coef[None, :]), "isMultinomial": False}
    md = sf.read_metadata(tmp_path / "bin")
    assert md["class"] == "org.apache.spark.ml.classification.LogisticRegressionModel" and md["paramMap"] == {}
    assert list(md["defaultParamMap"]) == list(LogisticRegressionModel._DEFAULT_ORDER)
    assert md["defaultParamMap"]["probabilityCol"] == "probability" and md["defaultParamMap"]["threshold"] == 0.5


# ---------------------------------------------------------------------------------------------- 10. serving
# letters only: cleaning drops digits
WORDS = [[f"{name}{chr(97 + i)}" for i in range(12)] for name in ("bank", "prize")]
COMMON = [f"talk{chr(97 + i // 26)}{chr(97 + i % 26)}" for i in range(40)]


@functools.lru_cache(maxsize=None)
def dialogues():
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    rng = np.random.default_rng(41)
    n = 380
    y = rng.integers(0, 2, size=n)
    texts = []
    for c in y:
        own = rng.choice(WORDS[c], size=rng.integers(1, 4))
        other = rng.choice(WORDS[1 - c], size=int(rng.random() < 0.15))
        words = np.concatenate([rng.choice(COMMON, size=rng.integers(8, 30)), own, other])
        texts.append(" ".join(rng.permutation(words)))
    raw = TextColumn(texts)
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.astype(np.float64)})
    return df.take_rows(np.arange(300)), df.take_rows(np.arange(300, n))


@functools.lru_cache(maxsize=None)
def pipeline_model():
    from fraud_detection_spark_kafka_llm_amd.ml import IDF, HashingTF, LinearSVC, Pipeline, StopWordsRemover, Tokenizer

    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
              IDF(inputCol="raw_features", outputCol="features"),
              LinearSVC(featuresCol="features", labelCol="labels", regParam=0.01, maxIter=40, threshold=0.25)]
    return Pipeline(stages=stages).fit(dialogues()[0])


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


def test_pipeline_fused_transform_equals_staged_and_round_trips(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import LinearSVCModel, PipelineModel

    train, test = dialogues()
    model = pipeline_model()
    svc = model.stages[-1]
    assert isinstance(svc, LinearSVCModel) and svc.numFeatures == 4096 and svc.getThreshold() == 0.25
    for df in (train, test):
        fused = model.transform(df)
        staged, _ = staged_outputs(model, df)
        assert "probability" not in fused.columns and "probability" not in staged.columns
        for name in ("rawPrediction", "prediction"):
            assert np.array_equal(bits(column(fused, name)), bits(column(staged, name))), name
    acc = float((column(model.transform(test), "prediction") == column(test, "labels")).mean())
    print(f"held-out accuracy {acc:.4f}")
    assert acc > 0.9
    path = tmp_path / "svc_pipeline"
    model.save(str(path))
    assert sf.verify_tree(path) == []
    back = PipelineModel.load(str(path))
    a, b = svc, back.stages[-1]
    assert isinstance(b, LinearSVCModel) and sf.read_metadata(path / "stages" / f"4_{a.uid}")["class"].endswith("LinearSVCModel")
    assert np.array_equal(bits(a.coefficients), bits(b.coefficients)) and a.intercept == b.intercept
    assert a._paramMap == b._paramMap and a._defaultParamMap == b._defaultParamMap
    for name in ("rawPrediction", "prediction"):
        assert np.array_equal(bits(column(model.transform(test), name)), bits(column(back.transform(test), name)))


@pytest.mark.parametrize("dev", DEVICES)
def test_model_serves_through_the_single_launch_paths(dev, tmp_path):
    from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
    from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM
    from fraud_detection_spark_kafka_llm_amd.stream import fake_kafka
    from fraud_detection_spark_kafka_llm_amd.stream.engine import StreamingEngine

    model, test = pipeline_model(), dialogues()[1]
    svc = model.stages[-1]
    thr = svc.getThreshold()
    texts = list(test.column("dialogue").strings)
    fp = model.compile(device=dev)
    pred, conf, rp = (t.cpu().numpy() for t in fp.predict(texts, clean=True))
    m = rp[:, 1]
    sig = 1.0 / (1.0 + np.exp(-(m - thr)))
    assert np.array_equal(bits(rp[:, 0]), bits(-m)) and np.array_equal(pred, (m > thr).astype(np.float64))
    np.testing.assert_allclose(conf[:, 1], sig, rtol=4 * 2.0 ** -52)
    assert np.array_equal(conf[:, 1] > 0.5, pred == 1.0) and {0.0, 1.0} == set(pred.tolist())
    # the single launch scores the fp32 values of its own CSR: the staged fp64 margin within that rounding
    staged, vc = staged_outputs(model, test)
    d = column(staged, "rawPrediction")[:, 1]
    ip, ix, v = (t.cpu().numpy() for t in vc.csr())
    mag = np.array([np.abs(v[a:e]) @ np.abs(svc.coefficients[ix[a:e]]) for a, e in zip(ip[:-1], ip[1:])])
    assert np.all(np.abs(m - d) <= 2.0 ** -23 * mag + (np.diff(ip) + 3) * 2.0 ** -52 * (mag + abs(svc.intercept)))
    # the agent
    model.save(str(tmp_path / "m"))
    agent = ClassificationAgent(str(tmp_path / "m"), llm=StubLLM(), device=dev)
    labels = agent.predict_batch(texts)
    for i in (0, 1, 2):
        got = agent.predict_and_get_label(texts[i])
        assert got == labels[i] and got["prediction"] == pred[i] and got["confidence"] == pytest.approx(sig[i], rel=1e-12)
    assert [r["prediction"] for r in labels] == pred.tolist()
    words = agent.contributing_words(texts[0], n=5)
    w = svc.coefficients
    assert len(words) == 5 and all(e["contribution"] == e["value"] * w[e["feature"]] for e in words)
    c = svc.contributions(vc.to(dev))
    cip, _, cv = (t.cpu().numpy() for t in c.csr())
    np.testing.assert_allclose(np.add.reduceat(cv, cip[:-1]), d, rtol=0, atol=1e-12)
    # the engine over the in-memory broker
    url = f"memory://linear-svc-{dev.replace(':', '-')}"
    broker = fake_kafka.broker_for(url)
    broker.create_topic("in", 3)
    p = fake_kafka.Producer({"bootstrap.servers": url})
    for i, t in enumerate(texts):
        p.produce("in", key=f"k{i}", value=json.dumps({"text": t}))
    cons = fake_kafka.Consumer({"bootstrap.servers": url, "group.id": "g", "auto.offset.reset": "earliest",
                                "enable.auto.commit": False})
    cons.subscribe(["in"])
    eng = StreamingEngine.from_agent(agent, cons, fake_kafka.Producer({"bootstrap.servers": url}), "out", batch_max=32,
                                     max_latency_ms=1)
    st = eng.run(max_messages=len(texts), idle_timeout_s=0.3)
    assert st["messages"] == len(texts) and st["produced"] == len(texts) and st["delivery_errors"] == 0
    recs = {msg.key(): json.loads(msg.value()) for msg in broker.messages("out")}
    for i, t in enumerate(texts):
        r = recs[f"k{i}".encode()]
        assert r["original_text"] == t and r["prediction"] == pred[i], i
        assert r["confidence"] == pytest.approx(sig[i], rel=1e-12), i


# ---------------------------------------------------------------------------------------------- 11. the CLI
def test_train_cli_fits_a_linear_svc_on_request(tmp_path):
    from fraud_detection_spark_kafka_llm_amd import train

    common = ["--data", "", "--synthetic", "300", "--no-plots", "--num-trees", "2", "--max-depth", "2", "--device", "cpu"]
    summary = train.main(common + ["--out-dir", str(tmp_path / "a"), "--linear-svc"])
    assert summary["LinearSVC"]["Test"]["Accuracy"] > 0.8
    assert set(summary["LinearSVC"]["Test"]) == {"Accuracy", "Precision", "Recall", "F1", "AUC"}
    with_flag = json.loads((tmp_path / "a" / "results.json").read_text())
    plain = train.main(common + ["--out-dir", str(tmp_path / "b")])
    without = json.loads((tmp_path / "b" / "results.json").read_text())
    assert "LinearSVC" not in train.make_classifiers() and list(plain) == list(train.make_classifiers())
    assert list(without) == ["metrics", "word_stats", "split"] and list(without["metrics"]) == list(train.make_classifiers())
    # every other output is unchanged by the flag
    assert {k: v for k, v in with_flag["metrics"].items() if k != "LinearSVC"} == without["metrics"]
    assert with_flag["word_stats"] == without["word_stats"] and with_flag["split"] == without["split"]


# ---------------------------------------------------------------------------------------------- 12. self-test
def test_svc_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--svc-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "svc selftest ok" in res.stdout
