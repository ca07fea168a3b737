"""ClusteringEvaluator and models.silhouette.silhouette. Unweighted, the per-row coefficients and the
value are compared with scikit-learn's silhouette_samples, a reference that shares nothing with
this code; weighted runs with the NumPy oracle of the contract only (scikit-learn has no weights, and
duplicating rows is another quantity: N - w against N - 1). Host, device and the worlds 2 and 3 must
give the same integers."""
import functools
import math

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.models.silhouette import silhouette
from fraud_detection_spark_kafka_llm_amd.ops import sparse
from test_clustering_ops import DEVICES, F, bits, oracle_group, oracle_sil, padded, to_vc

MEASURES = ["squaredEuclidean", "cosine"]
N, DIM, BLOBS = 60, 12, 3


@functools.lru_cache(maxsize=None)
def gaussians(dtype_name="float64"):
    """60 x 12 Gaussian rows around three means, stored as a CSR over 12 of the F features, and a
    prediction that follows the blobs but for a few rows."""
    rng = np.random.default_rng(11)
    cols = np.sort(rng.choice(F, DIM, replace=False)).astype(np.int32)
    blob = np.arange(N) % BLOBS
    means = rng.normal(0.0, 3.0, (BLOBS, DIM))
    X = (means[blob] + rng.normal(0.0, 1.0, (N, DIM))).astype(np.dtype(dtype_name))
    pred = blob.copy()
    pred[[4, 17, 40]] = (pred[[4, 17, 40]] + 1) % BLOBS
    csr = (np.arange(N + 1, dtype=np.int64) * DIM, np.tile(cols, N), X.reshape(-1))
    return csr, X.astype(np.float64), pred.astype(np.int32)


def weights_of(n):
    return np.random.default_rng(8).uniform(0.4, 2.6, n)


def oracle_silhouette(csr, w, pred, measure):
    """The evaluator's contract in NumPy: (value, silq, wq, s [n])."""
    m = "cosine" if measure == "cosine" else "euclidean"
    ip, ix, v = csr
    n, G = len(ip) - 1, int(pred.max()) + 1
    K = max(2, G)
    wmax = 1.0 if w is None else float(w.max())
    vmax = float(np.abs(v).max())
    xnmax = max(float(np.sqrt((v[ip[r]:ip[r + 1]].astype(np.float64) ** 2).sum())) for r in range(n)) ** 2
    cos = m == "cosine"
    k = sparse.nb_scale_exponent(wmax if cos else wmax * vmax, n)
    kw = sparse.nb_scale_exponent(wmax, n)
    kc = sparse.nb_scale_exponent(wmax if cos else wmax * xnmax, n)
    ks = sparse.nb_scale_exponent(2.0 * wmax, n)
    Kp = padded(K)
    S, Wq, cnt, costq, flag, _, _ = oracle_group(csr, w, pred, 1, G, np.zeros((F, Kp)), np.zeros(Kp), m, k, kw, kc)
    assert flag == 0
    MT, psi, nw, cnt32 = np.zeros((F, Kp)), np.zeros(Kp), np.zeros(Kp), np.zeros(Kp, dtype=np.int32)
    nw[:K] = np.ldexp(Wq.astype(np.float64), -kw)
    cnt32[:K] = cnt
    for c in range(K):
        if Wq[c]:
            MT[:, c] = np.ldexp(S[c].astype(np.float64), -k) / nw[c]
            psi[c] = 0.0 if cos else math.ldexp(float(costq[c]), -kc) / nw[c]
    silq, wq, flag, s, _ = oracle_sil(csr, w, pred, K, (MT, psi, nw, cnt32), m, ks, kw)
    assert flag == 0
    return math.ldexp(float(silq), -ks) / math.ldexp(float(wq), -kw), silq, wq, s


def run(csr, w, pred, measure, dev, **kw_):
    return silhouette(to_vc(csr, dev), torch.from_numpy(pred), None if w is None else torch.from_numpy(w), measure,
                      device=dev, want_rows=True, **kw_)


# 16 x the largest |NumPy oracle - scikit-learn| over the per-row coefficients and the value of the
# cases below, measured on the CPU with the oracle alone (scikit-learn 1.7.2): squaredEuclidean
# 1.677e-14 (fp64 input) and 2.899e-14 (fp32 input), cosine 1.417e-13 and 1.661e-13, each rounded
# up; the floor is 1e-15. The error is the contract's, not the summation's: every term of a cluster's coordinate sum
# is rounded to a multiple of 2^-k (k = 40 here, so up to 4.5e-13 a term) before the mean is taken.
MEASURED = {"squaredEuclidean": 2.899e-14, "cosine": 1.661e-13}
SKLEARN_TOL = {m: max(16 * e, 1e-15) for m, e in MEASURED.items()}


def sklearn_reference(X, pred, measure):
    from sklearn.metrics import silhouette_samples

    s = silhouette_samples(X, pred, metric="sqeuclidean" if measure == "squaredEuclidean" else "cosine")
    return s, float(np.mean(s))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_the_oracle_agrees_with_scikit_learn_within_the_recorded_error(measure, dtype_name):
    """The measurement behind SKLEARN_TOL, kept as a test: the code is not involved."""
    csr, X, pred = gaussians(dtype_name)
    value, _, _, s = oracle_silhouette(csr, None, pred, measure)
    ref_s, ref_value = sklearn_reference(X, pred, measure)
    worst = max(float(np.abs(s - ref_s).max()), abs(value - ref_value))
    print(f"{measure} {dtype_name}: max |oracle - scikit-learn| = {worst:.3e}")
    assert worst <= MEASURED[measure]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_unweighted_equals_scikit_learn_and_the_oracle(dtype_name, measure, dev):
    csr, X, pred = gaussians(dtype_name)
    res = run(csr, None, pred, measure, dev)
    ref_s, ref_value = sklearn_reference(X, pred, measure)
    s = res["s"].cpu().numpy()
    print(f"{measure} {dtype_name}: max |s - scikit-learn| = {np.abs(s - ref_s).max():.3e}, "
          f"|value - scikit-learn| = {abs(res['value'] - ref_value):.3e}")
    assert np.all(np.abs(s - ref_s) <= SKLEARN_TOL[measure]) and abs(res["value"] - ref_value) <= SKLEARN_TOL[measure]
    assert res["k"] == BLOBS and res["cnt"] == np.bincount(pred).tolist() and 0.3 < res["value"] < 1.0
    value, silq, wq, want_s = oracle_silhouette(csr, None, pred, measure)
    assert (res["silq"], res["wq"]) == (silq, wq) and bits(res["value"]) == bits(value)
    assert np.array_equal(bits(s), bits(want_s))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_weighted_equals_the_oracle_and_the_host(measure, dev):
    csr, _, pred = gaussians()
    w = weights_of(N)
    res = run(csr, w, pred, measure, dev)
    value, silq, wq, want_s = oracle_silhouette(csr, w, pred, measure)
    assert (res["silq"], res["wq"]) == (silq, wq) and bits(res["value"]) == bits(value)
    assert np.array_equal(bits(res["s"].cpu().numpy()), bits(want_s))
    host = run(csr, w, pred, measure, "cpu", threads=3)
    assert all(res[key] == host[key] for key in ("silq", "wq", "cnt", "Wq", "costq", "ek", "ekw", "ekc", "eks"))
    unweighted = run(csr, None, pred, measure, dev)
    assert unweighted["silq"] != res["silq"]


@pytest.mark.parametrize("dev", DEVICES)
def test_a_singleton_and_an_absent_cluster(dev):
    csr, _, pred = gaussians()
    pred = pred.copy()
    pred[pred == 1] = 5                                    # clusters 1, 3 and 4 are absent
    pred[7] = 3                                            # the only row of cluster 3
    res = run(csr, None, pred, "squaredEuclidean", dev)
    value, silq, wq, want_s = oracle_silhouette(csr, None, pred, "squaredEuclidean")
    assert res["k"] == 6 and res["cnt"][1] == 0 and res["cnt"][3] == 1 and float(res["s"][7]) == 0.0
    assert (res["silq"], res["wq"]) == (silq, wq) and np.array_equal(bits(res["s"].cpu().numpy()), bits(want_s))


# ---------------------------------------------------------------------------------------------- data parallel
DP_CASES = (("squaredEuclidean", False), ("squaredEuclidean", True), ("cosine", True))


def _dp_weights():
    w = weights_of(N)
    w[-2] = 3.25                                          # only the last shard holds the largest weight
    return w


def _dp_prediction():
    pred = gaussians("float32")[2].copy()
    pred[-1] = 4                                           # only the last shard sees the largest prediction
    pred[-5] = 4
    return pred


def _dp_result(res):
    return res["silq"], res["wq"], res["value"].hex(), res["k"], res["cnt"], res["Wq"], res["costq"], res["eks"]


def _dp_eval(rank, world):
    """Every case in one process group: a spawn costs more than the evaluations."""
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    (ip, ix, v), _, _ = gaussians("float32")
    pred, w = _dp_prediction(), _dp_weights()
    lo, hi = shard_range(N, rank, world)
    shard = (ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], v[ip[lo]:ip[hi]])
    return [_dp_result(run(shard, w[lo:hi] if weighted else None, pred[lo:hi], measure, "cpu"))
            for measure, weighted in DP_CASES]


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    outs = spawn(_dp_eval, world, backend="gloo")
    assert all(o == outs[0] for o in outs)
    csr = gaussians("float32")[0]
    for (measure, weighted), got in zip(DP_CASES, outs[0]):
        single = run(csr, _dp_weights() if weighted else None, _dp_prediction(), measure, "cpu")
        assert got == _dp_result(single), (measure, weighted)
        assert single["k"] == 5 and single["cnt"][3] == 0


# ---------------------------------------------------------------------------------------------- API
def test_defaults_are_sparks():
    from fraud_detection_spark_kafka_llm_amd.ml import ClusteringEvaluator

    ev = ClusteringEvaluator()
    assert (ev.getPredictionCol(), ev.getFeaturesCol(), ev.getMetricName(), ev.getDistanceMeasure()) == \
        ("prediction", "features", "silhouette", "squaredEuclidean")
    assert not ev.isSet("weightCol") and ev.isLargerBetter()


def test_evaluator_reads_the_frame():
    from fraud_detection_spark_kafka_llm_amd.ml import ClusteringEvaluator, Frame

    csr, _, pred = gaussians()
    w = weights_of(N)
    df = Frame({"features": to_vc(csr, "cpu"), "prediction": torch.from_numpy(pred), "p2": pred.astype(np.float64), "w": w})
    assert bits(ClusteringEvaluator().evaluate(df)) == bits(run(csr, None, pred, "squaredEuclidean", "cpu")["value"])
    ev = ClusteringEvaluator(predictionCol="p2", distanceMeasure="cosine", weightCol="w")
    assert bits(ev.evaluate(df)) == bits(run(csr, w, pred, "cosine", "cpu")["value"])
    with pytest.raises(ValueError):
        ClusteringEvaluator(distanceMeasure="euclidean").evaluate(df)
    with pytest.raises(ValueError):
        ClusteringEvaluator(metricName="daviesBouldin").evaluate(df)


@pytest.mark.parametrize("dev", DEVICES)
def test_bad_clusterings_and_bad_input_raise(dev):
    csr, _, pred = gaussians()
    ip, ix, v = csr
    with pytest.raises(ValueError, match="64"):
        run(csr, None, np.where(np.arange(N) == 3, 64, pred).astype(np.int32), "squaredEuclidean", dev)
    with pytest.raises(ValueError, match="two non-empty"):
        run(csr, None, np.zeros(N, dtype=np.int32), "squaredEuclidean", dev)
    with pytest.raises(ValueError, match="two non-empty"):
        run(csr, None, np.full(N, 7, dtype=np.int32), "cosine", dev)
    with pytest.raises(ValueError):
        run(csr, None, np.where(np.arange(N) == 3, -1, pred).astype(np.int32), "squaredEuclidean", dev)
    with pytest.raises(ValueError):
        silhouette(to_vc(csr, dev), torch.from_numpy(pred.astype(np.float64) + 0.5), device=dev)
    with pytest.raises(ValueError):
        silhouette(to_vc(csr, dev), torch.from_numpy(pred[:-1]), device=dev)
    with pytest.raises(ValueError):
        run(csr, None, pred, "manhattan", dev)
    for bad_w in (0.0, -1.0, float("nan"), float("inf")):
        w = weights_of(N)
        w[9] = bad_w
        with pytest.raises(ValueError):
            run(csr, w, pred, "squaredEuclidean", dev)
    for bad in (F, -1):
        bad_ix = ix.copy()
        bad_ix[30] = bad
        with pytest.raises(ValueError):
            run((ip, bad_ix, v), None, pred, "squaredEuclidean", dev)
    bad_v = v.copy()
    bad_v[30] = float("nan")
    with pytest.raises(ValueError):
        run((ip, ix, bad_v), None, pred, "squaredEuclidean", dev)
    zero_row = v.copy()
    zero_row[ip[5]:ip[6]] = 0.0
    with pytest.raises(ValueError):
        run((ip, ix, zero_row), None, pred, "cosine", dev)
    assert math.isfinite(run((ip, ix, zero_row), None, pred, "squaredEuclidean", dev)["value"])
    if dev != "cpu":
        torch.cuda.synchronize()
