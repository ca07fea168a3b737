"""Naive Bayes (csrc/nb_*.{h,hip,cpp}, ops.sparse.nb_sums / score_csr, models/nb.py, ml.NaiveBayes and its
users). The oracle below writes the contract of the README's "Naive Bayes" section in NumPy: one fp64
multiply and one ties-to-even rounding per term, Python integers for the sums, ``lane_sum`` for the
scores. Sums, models and scores are compared bit for bit."""
import functools
import math
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.models import nb as NB
from fraud_detection_spark_kafka_llm_amd.ops import sparse
from fraud_detection_spark_kafka_llm_amd.ops.text import ClassLinearScorer

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda", id="device", marks=pytest.mark.gpu)]
F = 4096
LIM = sparse.nb_limits()
CHUNK, MAXC = LIM["chunk_rows"], LIM["max_classes"]
EDGE_LENS = [0, 1, 63, 64, 65, 129]
EVERY, ONCE = 7, np.arange(4000, 4012)        # a feature of every non-empty row; features stored once


# ---------------------------------------------------------------------------------------------- oracle
def lane_sum(terms: np.ndarray) -> float:
    """Lane l adds terms l, l + 64, ... in ascending order; then v[:32] + v[32:], v[:16] + v[16:], ..."""
    p = np.zeros(64)
    t = np.zeros((len(terms) + 63) // 64 * 64)
    t[:len(terms)] = terms
    for blk in t.reshape(-1, 64):
        p = p + blk
    while p.size > 1:
        h = p.size // 2
        p = p[:h] + p[h:]
    return float(p[0])


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def scale_exponent(tmax: float, n: int) -> int:
    e = math.frexp(max(tmax, 1.0))[1]
    return min(40, 61 - int(n).bit_length() - e)


@functools.lru_cache(maxsize=None)
def corpus(n, num_classes, dtype_name, weighted, counts=True, seed=3):
    """CSR rows (the edge lengths first), labels that leave class 1 without rows when C > 2, weights."""
    rng = np.random.default_rng(seed + n)
    lens = np.array(EDGE_LENS + list(rng.integers(0, 13, n - len(EDGE_LENS))))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    rows = []
    for m in lens:
        ids = rng.choice(3900, size=m, replace=False) + 8
        if m:
            ids[0] = EVERY
        rows.append(np.sort(ids))
    once_rows = rng.choice(np.nonzero(lens >= 2)[0], size=len(ONCE), replace=False)
    for f, r in zip(ONCE, once_rows):
        rows[r][-1] = f                                   # the largest id of its row
    idx = np.concatenate(rows).astype(np.int32)
    nnz = int(indptr[-1])
    val = (rng.integers(1, 6, nnz) if counts else rng.uniform(0.05, 3.0, nnz)).astype(np.dtype(dtype_name))
    classes = [c for c in range(num_classes) if c != 1 or num_classes == 2]
    y = rng.choice(classes, size=n).astype(np.float64)
    y[-1] = num_classes - 1
    w = rng.uniform(0.3, 1.9, n) if weighted else None
    return (indptr, idx, val), y, w


def to_vc(csr, dev, size=F) -> VectorColumn:
    ip, ix, v = csr
    return VectorColumn(size, *(torch.from_numpy(np.array(a)).to(dev) for a in (ip, ix, v)))


def exponents(csr, w, n=None):
    n = len(csr[0]) - 1 if n is None else n
    wmax = float(w.max()) if w is not None else 1.0
    vmax = float(csr[2].astype(np.float64).max()) if len(csr[2]) else 0.0
    return scale_exponent(wmax * vmax, n), scale_exponent(wmax, n)


def oracle_sums(csr, y, w, num_classes, k, kw, size=F):
    """(S [C, F], Wq [C], cnt [C]) with Python integers, as int64 arrays."""
    ip, ix, v = csr
    n = len(y)
    ww = np.ones(n) if w is None else w
    row = np.repeat(np.arange(n), np.diff(ip))
    q = np.rint(np.ldexp(ww[row] * v.astype(np.float64), k)).astype(np.int64)
    S = np.zeros((num_classes, size), dtype=object)
    np.add.at(S, (y[row].astype(np.int64), ix), q.astype(object))
    Wq = np.zeros(num_classes, dtype=object)
    np.add.at(Wq, y.astype(np.int64), np.rint(np.ldexp(ww, kw)).astype(np.int64).astype(object))
    cnt = np.bincount(y.astype(np.int64), minlength=num_classes)
    assert all(abs(int(x)) < 2 ** 61 for x in S.reshape(-1))
    return S.astype(np.int64), Wq.astype(np.int64), cnt.astype(np.int64)


def oracle_finalize(S, Wq, k, kw, lam, model_type, size=F):
    C = len(Wq)
    n = np.array([float(int(x)) * 2.0 ** -kw for x in Wq])
    total = float(sum(int(x) for x in Wq)) * 2.0 ** -kw
    pi = np.log(n + lam) - np.log(total + C * lam)
    num = np.log(S.astype(np.float64) * 2.0 ** -k + lam)
    if model_type == "multinomial":
        den = np.log(np.array([float(sum(int(x) for x in S[c])) * 2.0 ** -k for c in range(C)]) + size * lam)
    else:
        den = np.log(n + 2 * lam)
    return pi, num - den[:, None]


def run_sums(csr, y, w, C, k, kw, dev, **kw_):
    S, Wq, cnt = sparse.nb_sums(to_vc(csr, dev), torch.from_numpy(y), None if w is None else torch.from_numpy(w),
                                C, k, kw, **kw_)
    assert S.dtype == Wq.dtype == cnt.dtype == torch.int64 and S.shape == (C, F)
    return S.numpy(), Wq.numpy(), cnt.numpy()


def check_sums(csr, y, w, C, dev, **kw_):
    k, kw = exponents(csr, w)
    want = oracle_sums(csr, y, w, C, k, kw)
    got = run_sums(csr, y, w, C, k, kw, dev, **kw_)
    for g, t in zip(got, want):
        assert np.array_equal(g, t)
    return want


# ---------------------------------------------------------------------------------------------- 1. sums
def test_limits_are_exported():
    assert set(LIM) >= {"max_classes", "chunk_rows", "table_bytes", "max_table_bytes", "k_max", "sum_bits", "wave",
                        "block", "prefix_rows"}
    assert MAXC == 8 and LIM["k_max"] == 40 and LIM["sum_bits"] == 61 and LIM["wave"] == 64
    assert 0 < LIM["table_bytes"] <= LIM["max_table_bytes"] < 64 * 1024


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_sums_equal_the_oracle_around_the_row_chunk(n, dev):
    csr, y, w = corpus(n, 3, "float64", True, counts=False)
    S, _, cnt = check_sums(csr, y, w, 3, dev)
    assert cnt[1] == 0 and not S[1].any()                 # a class without rows
    assert np.count_nonzero(S[:, ONCE]) == len(ONCE)      # features stored once


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_sums_equal_the_oracle(C, dtype_name, weighted, dev):
    csr, y, w = corpus(CHUNK + 1, C, dtype_name, weighted, counts=not weighted)
    check_sums(csr, y, w, C, dev)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_hot_set_and_threads_change_no_bit(C, dev):
    csr, y, w = corpus(2 * CHUNK + 3, C, "float32", True, counts=False)
    slots = LIM["table_bytes"] // (8 * C)
    full = np.unique(np.concatenate([[EVERY], ONCE, np.arange(slots)]))[:slots]      # every slot taken
    assert len(full) == slots and EVERY in full
    for hot in ([], full, None, np.arange(LIM["max_table_bytes"] // (8 * C))):
        check_sums(csr, y, w, C, dev, hot=hot)
    for threads in (1, 7):
        check_sums(csr, y, w, C, dev, threads=threads)
    check_sums(csr, y, w, C, dev, chunk_rows=5)
    if dev == "cuda":
        with pytest.raises(ValueError):
            check_sums(csr, y, w, C, dev, hot=np.arange(LIM["max_table_bytes"] // (8 * C) + 1))


# ---------------------------------------------------------------------------------------------- 2. fixed point
@pytest.mark.parametrize("dev", DEVICES)
def test_integer_counts_sum_exactly(dev):
    csr, y, _ = corpus(CHUNK + 1, 3, "float32", False, counts=True)
    k, kw = exponents(csr, None)
    S, Wq, cnt = run_sums(csr, y, None, 3, k, kw, dev)
    ip, ix, v = csr
    row = np.repeat(np.arange(len(y)), np.diff(ip))
    counts = np.zeros((3, F), dtype=np.int64)
    np.add.at(counts, (y[row].astype(np.int64), ix), v.astype(np.int64))
    assert np.array_equal(S, counts << k) and np.array_equal(S.astype(np.float64) * 2.0 ** -k, counts)
    assert np.array_equal(Wq, cnt << kw) and np.array_equal(cnt, np.bincount(y.astype(np.int64), minlength=3))


@pytest.mark.parametrize("dev", DEVICES)
def test_rounding_error_is_half_an_ulp_of_the_scale_per_term(dev):
    csr, y, w = corpus(300, 2, "float64", True, counts=False)
    k, kw = exponents(csr, w)
    S, _, _ = run_sums(csr, y, w, 2, k, kw, dev)
    ip, ix, v = csr
    row = np.repeat(np.arange(len(y)), np.diff(ip))
    exact, terms = {}, {}
    for r, f, x in zip(row, ix, v):
        key = (int(y[r]), int(f))
        exact[key] = exact.get(key, 0) + Fraction(float(w[r] * x))       # t_ij is one fp64 multiply
        terms[key] = terms.get(key, 0) + 1
    for (c, f), t in exact.items():
        assert abs(Fraction(int(S[c, f]), 2 ** k) - t) <= Fraction(terms[(c, f)], 2 ** (k + 1))
    assert int(np.count_nonzero(S)) == len(exact)


# ---------------------------------------------------------------------------------------------- 3. scale exponent
def test_scale_exponent_follows_the_formula():
    for n, want in ((2 ** 20 - 1, 40), (2 ** 20, 39), (1, 40), (2 ** 30, 29)):
        assert sparse.nb_scale_exponent(1.0, n) == scale_exponent(1.0, n) == want
    for tmax in (0.0, 0.3, 1.0, 1.5, 2.0, 1023.9, 1024.0, 3e5):
        for n in (1, 1000, 2 ** 20 - 1, 2 ** 20):
            assert sparse.nb_scale_exponent(tmax, n) == scale_exponent(tmax, n)
    assert sparse.nb_scale_exponent(2.0 ** 40 - 1, 2 ** 20) == 0
    with pytest.raises(ValueError):
        sparse.nb_scale_exponent(2.0 ** 40, 2 ** 20)
    with pytest.raises(ValueError):
        sparse.nb_scale_exponent(float("nan"), 10)


@pytest.mark.parametrize("n", [2 ** 20 - 1, 2 ** 20])
def test_fit_uses_the_exponents_of_its_row_count(n):
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[3:] = 2                                        # rows 0 and 1 are empty, row 2 holds two entries
    csr = (indptr, np.array([5, 9], dtype=np.int32), np.array([3.0, 1.0]))
    y = np.zeros(n)
    y[2::2] = 1.0
    w = np.full(n, 0.75)
    w[7] = 2.5
    res = NB.fit_naive_bayes(to_vc(csr, "cpu", 16), y, weights=w, device="cpu")
    assert (res["k"], res["kw"]) == (scale_exponent(7.5, n), scale_exponent(2.5, n))
    assert res["kw"] == (38 if n == 2 ** 20 else 39) and res["k"] == res["kw"] - 1
    tiny = (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([2.0 ** 60]))
    with pytest.raises(ValueError):
        NB.fit_naive_bayes(to_vc(tiny, "cpu", 4), np.array([1.0]), device="cpu")


# ---------------------------------------------------------------------------------------------- 4. model
@functools.lru_cache(maxsize=None)
def fitted(model_type, weighted, dev, lam=1.0, C=3):
    csr, y, w = corpus(CHUNK + 1, C, "float64", weighted, counts=True)
    if model_type == "bernoulli":
        csr = (csr[0], csr[1], np.ones_like(csr[2]))
    res = NB.fit_naive_bayes(to_vc(csr, dev), y, weights=w, smoothing=lam, model_type=model_type, device=dev)
    return csr, y, w, res


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("model_type", ["multinomial", "bernoulli"])
def test_fit_equals_finalize_of_the_oracle_sums(model_type, weighted, dev):
    csr, y, w, res = fitted(model_type, weighted, dev, 0.5)
    k, kw = exponents(csr, w)
    assert (res["k"], res["kw"], res["C"], res["F"]) == (k, kw, 3, F)
    S, Wq, cnt = oracle_sums(csr, y, w, 3, k, kw)
    pi, theta = oracle_finalize(S, Wq, k, kw, 0.5, model_type)
    assert np.array_equal(bits(res["pi"]), bits(pi)) and np.array_equal(bits(res["theta"]), bits(theta))
    fpi, ftheta = NB.finalize(S, Wq, k, kw, 0.5, model_type)
    assert np.array_equal(bits(fpi), bits(pi)) and np.array_equal(bits(ftheta), bits(theta))
    assert np.array_equal(res["cnt"], cnt)
    host = fitted(model_type, weighted, "cpu", 0.5)[3]             # host fit = device fit
    assert np.array_equal(bits(res["pi"]), bits(host["pi"])) and np.array_equal(bits(res["theta"]), bits(host["theta"]))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("lam", [1.0, 0.25])
def test_theta_matches_sklearn(lam, dev):
    import scipy.sparse as sp
    from sklearn.naive_bayes import BernoulliNB, MultinomialNB

    for model_type, cls, kw in (("multinomial", MultinomialNB, {}), ("bernoulli", BernoulliNB, {"binarize": None})):
        csr, y, _, res = fitted(model_type, False, dev, lam)
        X = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(len(y), F))
        # class 1 has no rows: sklearn names the classes it sees
        ref = cls(alpha=lam, **kw).fit(X, y)
        seen = ref.classes_.astype(int)
        assert np.abs(ref.feature_log_prob_).max() < 16
        assert np.abs(res["theta"][seen] - ref.feature_log_prob_).max() <= 1e-12
        n = np.bincount(y.astype(int), minlength=3).astype(np.float64)
        assert np.array_equal(bits(res["pi"]), bits(np.log(n + lam) - np.log(n.sum() + 3 * lam)))


def test_model_types_and_smoothing_are_checked():
    csr, y, _ = corpus(CHUNK - 1, 2, "float64", False)
    vc = to_vc(csr, "cpu")
    for mt in ("complement", "gaussian"):
        with pytest.raises(NotImplementedError):
            NB.fit_naive_bayes(vc, y, model_type=mt, device="cpu")
    with pytest.raises(ValueError):
        NB.fit_naive_bayes(vc, y, model_type="poisson", device="cpu")
    with pytest.raises(ValueError):
        NB.fit_naive_bayes(vc, y, smoothing=-0.5, device="cpu")


# ---------------------------------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("dev", DEVICES)
def test_bad_input_raises_before_any_model(dev):
    csr, y, w = corpus(CHUNK + 1, 3, "float64", True, counts=True)
    ip, ix, v = csr

    def fit(val=v, labels=y, weights=w, **kw):
        return NB.fit_naive_bayes(to_vc((ip, ix, val), dev), labels, weights=weights, device=dev, **kw)

    def changed(a, i, x):
        b = a.copy()
        b[i] = x
        return b

    fit()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fit(val=changed(v, 300, bad))
    with pytest.raises(ValueError):
        fit(model_type="bernoulli")                                   # counts above 1
    with pytest.raises(ValueError):
        fit(val=changed(np.ones_like(v), 300, 0.5), model_type="bernoulli")
    fit(val=changed(np.ones_like(v), 300, 0.0), model_type="bernoulli")
    for bad in (0.5, -1.0, float("nan"), float(MAXC)):
        with pytest.raises(ValueError):
            fit(labels=changed(y, 40, bad))
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fit(weights=changed(w, 40, bad))
    with pytest.raises(ValueError):
        fit(smoothing=-1.0)
    k, kw = exponents(csr, w)
    with pytest.raises(ValueError):
        run_sums(csr, y, w, MAXC + 1, k, kw, dev)
    with pytest.raises(ValueError):
        run_sums(csr, changed(y, 40, 3.0), w, 3, k, kw, dev)         # a label outside 0 .. C - 1


# ---------------------------------------------------------------------------------------------- 6. scores
def score_oracle(csr, W, b):
    ip, ix, v = csr
    v = v.astype(np.float64)
    return np.array([[lane_sum(v[a:e] * W[ix[a:e], c]) + b[c] for c in range(len(b))]
                     for a, e in zip(ip[:-1], ip[1:])]).reshape(len(ip) - 1, len(b))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("model_type,C", [("multinomial", 2), ("multinomial", 3), ("bernoulli", 3), ("multinomial", MAXC)])
def test_scores_equal_spmv_and_the_lane_order_oracle(model_type, C, dtype_name, dev):
    _, _, _, res = fitted(model_type, False, "cpu", 1.0, C)
    W, b = NB.class_linear(res["pi"], res["theta"], model_type)
    assert W.shape == (F, C) and b.shape == (C,)
    if model_type == "bernoulli":
        neg = np.log1p(-np.exp(res["theta"]))
        assert np.array_equal(bits(W), bits((res["theta"] - neg).T))
        assert np.array_equal(bits(b), bits([res["pi"][c] + math.fsum(neg[c]) for c in range(C)]))
    csr = corpus(140, C, dtype_name, False, counts=model_type == "bernoulli", seed=11)[0]
    if model_type == "bernoulli":
        csr = (csr[0], csr[1], np.ones_like(csr[2]))
    vc = to_vc(csr, dev)
    raw = sparse.score_csr(vc, ClassLinearScorer(W, b))
    assert raw.shape == (140, C) and raw.dtype == torch.float64
    raw = raw.cpu().numpy()
    want = score_oracle(csr, W, b)
    assert np.array_equal(bits(raw), bits(want))
    ip, ix, v = (t.contiguous() for t in vc.csr())
    for c in range(C):
        col = sparse.spmv(ip, ix.to(torch.int32), v, torch.from_numpy(np.ascontiguousarray(W[:, c])).to(dev)) + b[c]
        assert np.array_equal(bits(raw[:, c]), bits(col.cpu().numpy()))
    v64 = csr[2].astype(np.float64)
    for r, (a, e) in enumerate(zip(csr[0][:-1], csr[0][1:])):          # (n - 1) 2^-53 sum |term| of fsum
        for c in range(C):
            terms = np.append(v64[a:e] * W[csr[1][a:e], c], b[c])
            assert abs(raw[r, c] - math.fsum(terms)) <= (len(terms) - 1) * 2.0 ** -53 * np.abs(terms).sum()


def make_model(model_type="multinomial", C=3, **params):
    from fraud_detection_spark_kafka_llm_amd.ml import NaiveBayesModel

    res = fitted(model_type, False, "cpu", 1.0, C)[3]
    return NaiveBayesModel(res["pi"], res["theta"], modelType=model_type, **params)


@pytest.mark.parametrize("dev", DEVICES)
def test_probabilities_predictions_thresholds_and_ties(dev):
    m = make_model()
    csr = corpus(140, 3, "float64", False, seed=11)[0]
    raw = sparse.score_csr(to_vc(csr, dev), m.class_scorer())
    rp, prob, pred = (t.cpu().numpy() for t in m.postprocess(raw))
    raw = raw.cpu().numpy()
    e = np.exp(raw - raw.max(axis=1, keepdims=True))
    want = e / e.sum(axis=1, keepdims=True)
    assert np.array_equal(bits(rp), bits(raw))
    # exp of two libraries (<= 1 ulp each), the sum and the division: 4 ulp
    np.testing.assert_allclose(prob, want, rtol=4 * 2.0 ** -52, atol=0)
    assert np.array_equal(pred, np.argmax(prob, axis=1).astype(np.float64))
    assert len(set(pred.tolist())) > 1
    t = np.array([0.9, 1e-9, 0.05])
    mt = make_model(thresholds=t.tolist())
    pred_t = mt.postprocess(torch.from_numpy(raw))[2].numpy()
    assert np.array_equal(pred_t, np.argmax(prob / t, axis=1).astype(np.float64)) and not np.array_equal(pred_t, pred)
    ties = torch.tensor([[-3.0, -3.0, -3.0], [-5.0, -1.0, -1.0], [-2.0, -7.0, -2.0]], dtype=torch.float64, device=dev)
    assert m.postprocess(ties)[2].cpu().tolist() == [0.0, 1.0, 0.0]
    assert make_model(thresholds=[0.5, 0.25, 0.25]).postprocess(ties)[2].cpu().tolist() == [1.0, 1.0, 2.0]
    x = {int(f): float(v) for f, v in zip(csr[1][csr[0][5]:csr[0][6]], csr[2][csr[0][5]:csr[0][6]])}
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import SparseVector

    sv = SparseVector(F, sorted(x), [x[f] for f in sorted(x)])
    assert np.array_equal(bits(m.predictRaw(sv).toArray()), bits(raw[5])) and m.predict(sv) == pred[5]
    assert np.array_equal(bits(m.predictProbability(sv).toArray()), bits(m.postprocess(torch.from_numpy(raw[5:6]))[1][0]))
    assert m.numClasses == 3 and m.numFeatures == F and m.sigma.shape == (0, 0)
    with pytest.raises(ValueError, match="3 classes"):
        m.scorer()


# ---------------------------------------------------------------------------------------------- 7. ML API
@functools.lru_cache(maxsize=None)
def dialogues():
    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    pt, y = synth.generate(synth.SynthConfig(n=560, seed=31))
    raw = TextColumn(pt.strings())
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})
    return df.take_rows(np.arange(400)), df.take_rows(np.arange(400, 560))


def stages(**nb):
    from fraud_detection_spark_kafka_llm_amd.ml import IDF, HashingTF, NaiveBayes, StopWordsRemover, Tokenizer

    return [Tokenizer(inputCol="clean_text", outputCol="words"),
            StopWordsRemover(inputCol="words", outputCol="filtered_words"),
            HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
            IDF(inputCol="raw_features", outputCol="features"),
            NaiveBayes(featuresCol="features", labelCol="labels", **nb)]


@functools.lru_cache(maxsize=None)
def pipeline_model():
    from fraud_detection_spark_kafka_llm_amd.ml import Pipeline

    return Pipeline(stages=stages()).fit(dialogues()[0])


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
    nbm = model.stages[-1]
    assert type(nbm).__name__ == "NaiveBayesModel" and nbm.numClasses == 2 and nbm.numFeatures == 4096
    for df in (train, test):
        fused = model.transform(df)
        staged, _ = staged_outputs(model, df)
        for name in ("rawPrediction", "probability", "prediction"):
            assert np.array_equal(bits(column(fused, name)), bits(column(staged, name))), name
        assert column(fused, "rawPrediction").shape == (len(df), 2)
    y = column(test, "labels")
    acc = float((column(model.transform(test), "prediction") == y).mean())
    majority = max(y.mean(), 1 - y.mean())
    print(f"held-out accuracy {acc:.4f}, majority class {majority:.4f}")
    assert acc > 0.9 and acc > majority


def test_spark_layout_round_trip_is_bitwise(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import NaiveBayesModel, PipelineModel

    model = pipeline_model()
    path = tmp_path / "nb_pipeline"
    model.save(str(path))
    assert sf.verify_tree(path) == []
    back = PipelineModel.load(str(path))
    a, b = model.stages[-1], back.stages[-1]
    assert isinstance(b, NaiveBayesModel)
    assert sf.read_metadata(path / "stages" / f"4_{a.uid}")["class"] == "org.apache.spark.ml.classification.NaiveBayesModel"
    assert np.array_equal(bits(a.pi), bits(b.pi)) and np.array_equal(bits(a.theta), bits(b.theta))
    assert b.theta.shape == (2, 4096) and b.sigma.shape == (0, 0) and b.getSmoothing() == 1.0
    row = sf.read_data_parquet(path / "stages" / f"4_{a.uid}").to_pylist()[0]
    assert set(row) == {"pi", "theta", "sigma"} and row["theta"]["type"] == 1 and row["sigma"]["numRows"] == 0
    test = dialogues()[1]
    for name in ("rawPrediction", "probability", "prediction"):
        assert np.array_equal(bits(column(model.transform(test), name)), bits(column(back.transform(test), name)))
    multi = make_model(thresholds=[0.2, 0.3, 0.5])
    multi.save(str(tmp_path / "nb3"))
    again = NaiveBayesModel.load(str(tmp_path / "nb3"))
    assert again.numClasses == 3 and again.getThresholds() == [0.2, 0.3, 0.5]
    assert np.array_equal(bits(again.theta), bits(multi.theta))


def test_train_cli_adds_naive_bayes_on_request(tmp_path):
    from fraud_detection_spark_kafka_llm_amd import train

    common = ["--data", "", "--synthetic", "300", "--no-plots", "--num-trees", "2", "--max-depth", "2",
              "--out-dir", str(tmp_path), "--device", "cpu"]
    summary = train.main(common + ["--naive-bayes"])
    assert summary["NaiveBayes"]["Test"]["Accuracy"] > 0.9
    assert "NaiveBayes" not in train.make_classifiers()              # off by default


# ---------------------------------------------------------------------------------------------- 8. serving margin
def margin_reference(model, df):
    """raw_1 - raw_0 of Spark's rawPrediction, the derivable bound of a margin computed in one sum,
    and the NumPy prediction of every row."""
    staged, vc = staged_outputs(model, df)
    raw = column(staged, "rawPrediction")
    cs = model.stages[-1].class_scorer()
    ip, ix, v = (t.cpu().numpy() for t in vc.csr())
    mag = np.array([np.abs(v[a:e]) @ (np.abs(cs.W[ix[a:e], 0]) + np.abs(cs.W[ix[a:e], 1])) for a, e in zip(ip[:-1], ip[1:])])
    bound = 2 * (np.diff(ip) + 3) * 2.0 ** -53 * (mag + abs(cs.b[0]) + abs(cs.b[1]))
    return raw[:, 1] - raw[:, 0], bound, column(staged, "prediction"), vc


def test_margin_oracle_excludes_no_row():
    d, bound, pred, _ = margin_reference(pipeline_model(), dialogues()[1])
    assert np.all(np.abs(d) > bound) and np.array_equal(pred, (d > 0).astype(np.float64))


@pytest.mark.parametrize("dev", DEVICES)
def test_binary_model_serves_through_the_single_launch_paths(dev, tmp_path):
    from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
    from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import make_scorer
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    model, test = pipeline_model(), dialogues()[1]
    nbm = model.stages[-1]
    d, bound, pred_ref, vc = margin_reference(model, test)
    texts = list(test.column("dialogue").strings)
    clean = list(test.column("clean_text").strings)
    fp = model.compile(device=dev)
    m = fp.run(clean, clean=False).raw.cpu().numpy()
    assert m.shape == (len(texts), 1)
    print(f"max |m - (raw_1 - raw_0)| / bound = {(np.abs(m[:, 0] - d) / bound).max():.3e}")
    assert np.all(np.abs(m[:, 0] - d) <= bound)
    sure = np.abs(d) > bound
    assert (~sure).mean() <= 0.01
    pred, prob, rp = (t.cpu().numpy() for t in fp.predict(texts, clean=True))
    assert np.array_equal(bits(rp), bits(np.stack([np.zeros(len(m)), m[:, 0]], axis=1)))
    assert np.array_equal(pred[sure], pred_ref[sure])
    sig = 1.0 / (1.0 + np.exp(-m[:, 0]))
    np.testing.assert_allclose(prob[:, 1], sig, rtol=4 * 2.0 ** -52)
    np.testing.assert_allclose(prob[:, 0], 1.0 / (1.0 + np.exp(m[:, 0])), rtol=4 * 2.0 ** -52)
    # the agent
    model.save(str(tmp_path / "m"))
    agent = ClassificationAgent(str(tmp_path / "m"), llm=StubLLM(), device=dev)
    for i in (0, 1, 2):
        got = agent.predict_and_get_label(texts[i])
        assert got["prediction"] == pred[i] and got["confidence"] == pytest.approx(sig[i], rel=1e-12)
    words = agent.contributing_words(texts[0], n=5)
    w = nbm.scorer().w
    assert len(words) == 5 and all(e["contribution"] == e["value"] * w[e["feature"]] for e in words)
    # contributions: a row sums to the margin
    col = nbm.contributions(vc.to(dev))
    cp, cx, cv = (t.cpu().numpy() for t in col.csr())
    assert col.size == 4097 and np.array_equal(np.diff(cp), np.diff(vc.csr()[0].cpu().numpy()) + 1)
    sums = np.array([math.fsum(cv[a:e]) for a, e in zip(cp[:-1], cp[1:])])
    assert np.all(cx[cp[1:] - 1] == 4096) and np.all(np.abs(sums - d) <= bound)
    # the streaming scorer
    sc = make_scorer(fp.spec(True), fp.idf.idf, nbm.scorer(), dev, max_docs=256, max_bytes=256 * 4096)
    ring = PinnedRing(slots=1, max_docs=256, max_bytes=256 * 4096)
    ring.slots[0].fill(texts)
    sm = sc.score_packed(ring.slots[0])
    assert np.array_equal(bits(sm), bits(m))
    spred, sp1 = nbm.postprocess_numpy(np.array(sm))
    assert np.array_equal(spred[sure], pred_ref[sure]) and np.array_equal(spred, pred)
    np.testing.assert_allclose(sp1, sig, rtol=4 * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------- 9. data parallel
def _dp_corpus():
    csr, y, w = corpus(CHUNK + 1, 3, "float32", True, counts=False, seed=17)
    ip, ix, v = csr
    v, w = v.copy(), w.copy()
    v[-1], w[-2] = 4000.5, 3.25                           # only the last shard holds the maxima
    return (ip, ix, v), y, w


def _dp_fit(rank, world, model_type):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    (ip, ix, v), y, w = _dp_corpus()
    if model_type == "bernoulli":
        v = np.ones_like(v)
    lo, hi = shard_range(len(y), rank, world)
    shard = (ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], v[ip[lo]:ip[hi]])
    res = NB.fit_naive_bayes(to_vc(shard, "cpu"), y[lo:hi], weights=w[lo:hi], model_type=model_type, device="cpu")
    return res["pi"].tobytes(), res["theta"].tobytes(), res["k"], res["kw"]


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_fit_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    for model_type in ("bernoulli", "multinomial"):
        csr, y, w = _dp_corpus()
        if model_type == "bernoulli":
            csr = (csr[0], csr[1], np.ones_like(csr[2]))
        single = NB.fit_naive_bayes(to_vc(csr, "cpu"), y, weights=w, model_type=model_type, device="cpu")
        outs = spawn(_dp_fit, world, model_type, backend="gloo")
        assert all(o == outs[0] for o in outs)
        assert outs[0] == (single["pi"].tobytes(), single["theta"].tobytes(), single["k"], single["kw"])
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    (ip, _, v), _, w = _dp_corpus()
    lo, hi = shard_range(len(w), 0, world)                 # the first shard's own maxima pick another scale
    assert scale_exponent(float(w[lo:hi].max()) * float(v[ip[lo]:ip[hi]].max()), len(w)) == 40 != single["k"]


# ---------------------------------------------------------------------------------------------- 10. self-test
def test_nb_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--nb-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "nb_selftest: ok" in res.stdout
