"""Validation monitoring and early stopping of the GBDT trainer (models/monitor.py) and of
``SparkXGBClassifier(validation_indicator_col=..., early_stopping_rounds=...)``."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
from fraud_detection_spark_kafka_llm_amd.ml.base import Params
from fraud_detection_spark_kafka_llm_amd.ml.frame import Frame
from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import ensemble_arrays
from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier, SparkXGBClassifierModel
from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
from fraud_detection_spark_kafka_llm_amd.ops import native
from fraud_detection_spark_kafka_llm_amd.ops.sparse import score_csr
from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

GOLDEN = Path(__file__).resolve().parent / "golden" / "xgb_no_validation"
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
METRICS = ["auc", "logloss", "error"]
N_TRAIN, ROUNDS, PATIENCE = 4000, 60, 5
PARAMS = GBDTParams(n_estimators=ROUNDS, max_depth=4, learning_rate=0.3)


def _int_features(n: int, seed: int) -> tuple:
    """Integer features, value ranges of 9..24 distinct values (zero included, some negative so
    that the zero bin sits inside the range), and a noisy non-linear label."""
    rng = np.random.default_rng(seed)
    F = 10
    X = np.zeros((n, F))
    for f in range(F):
        lo = -(f % 4)
        hi = 8 + 2 * f if f < 8 else 12
        vals = rng.integers(lo, hi, n)
        keep = rng.random(n) < (0.55 + 0.04 * f)
        X[:, f] = np.where(keep, vals, 0)
    score = (1.3 * (X[:, 0] > 3) + 0.9 * (X[:, 2] * X[:, 5] > 20) - 0.8 * (X[:, 7] < 2) + 0.05 * X[:, 9]
             + 0.4 * np.sin(X[:, 4]))
    y = (score + rng.normal(0, 0.6, n) > 0.6).astype(np.float32)
    return X, y


def _csr_vc(X: np.ndarray) -> VectorColumn:
    nz = X != 0
    indptr = np.zeros(X.shape[0] + 1, dtype=np.int64)
    np.cumsum(nz.sum(1), out=indptr[1:])
    r, c = np.nonzero(nz)
    return VectorColumn(X.shape[1], torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int32)),
                        torch.from_numpy(X[r, c]))


def _sig(trees):
    return [(t.feature.tolist(), t.threshold.tolist(), t.stats.tolist()) for t in trees]


# ------------------------------------------------------------------------------- independent metrics
def np_auc(m, y):
    groups = {}
    for v, lab in zip(m.tolist(), y.tolist()):
        g = groups.setdefault(0.0 if v == 0.0 else v, [0, 0])
        g[1 if lab > 0.5 else 0] += 1
    u2 = nb = pos = 0
    for key in sorted(groups):
        rn, rp = groups[key]
        u2 += rp * (2 * nb + rn)
        nb += rn
        pos += rp
    return float(u2) / (2.0 * float(pos) * float(nb))


def np_error(m, y):
    p = 1.0 / (1.0 + np.exp(-m))
    return float(np.sum((p > 0.5) != (y > 0.5))) / float(len(y))


def np_logloss(m, y):
    terms = []
    for v, lab in zip(m.tolist(), y.tolist()):
        p = 1.0 / (1.0 + math.exp(-v))
        terms.append(-math.log(max(p, 1e-16)) if lab > 0.5 else -math.log(max(1.0 - p, 1e-16)))
    return math.fsum(terms) / len(terms)


NP_METRIC = {"auc": np_auc, "logloss": np_logloss, "error": np_error}


def logloss_bound(n, w_sum=None, w_max=1.0):
    k = int(native.lib().eval_sum_kexp(n, w_max))
    return 2.0 ** -(k + 1) * n / (w_sum if w_sum is not None else n) + 1e-13


class Data:
    """The shared inputs and the plain 60-round fit on the training rows alone; its per-round
    validation margins (sequential ``score_csr(..., cmp_less=True)`` sums) give every expected
    value of the tests below. Computed once per device and never changed."""
    _cache: dict = {}

    def __init__(self, device):
        X, y = _int_features(6000, 11)
        self.X, self.y = X, y
        self.tr, self.ytr = _csr_vc(X[:N_TRAIN]), torch.from_numpy(y[:N_TRAIN])
        self.va, self.yva = _csr_vc(X[N_TRAIN:]), torch.from_numpy(y[N_TRAIN:])
        self.plain = fit_gbdt(self.tr, self.ytr, PARAMS, device=device)
        m = np.full(len(self.yva), self.plain.base_margin)
        self.margins = []
        for t in self.plain.trees:
            m = m + score_csr(self.va, ensemble_arrays([t], "value", cmp_less=True))[:, 0].numpy()
            self.margins.append(m)
        yv = y[N_TRAIN:]
        self.expected = {k: [fn(mm, yv) for mm in self.margins] for k, fn in NP_METRIC.items()}

    @classmethod
    def get(cls, device):
        if device not in cls._cache:
            cls._cache[device] = cls(device)
        return cls._cache[device]

    def best(self, metric):
        """(best_iteration, the round the fit stops at) from the expected history."""
        h = self.expected[metric]
        best = 0
        for t in range(1, len(h)):
            if (h[t] > h[best]) if metric == "auc" else (h[t] < h[best]):
                best = t
            if t - best >= PATIENCE:
                return best, t
        return best, len(h) - 1


# ------------------------------------------------------------------------------- 1. the validation margin
@pytest.mark.parametrize("device", DEVICES)
def test_monitored_margin_equals_sequential_scorer_sum(device):
    X, y = _int_features(6000, 11)
    tr, va = _csr_vc(X[:N_TRAIN]), _csr_vc(X[N_TRAIN:])
    from fraud_detection_spark_kafka_llm_amd.models import monitor

    seen = []
    orig = monitor.ValidationMonitor.queue

    def spy(self, t):
        seen.append(self.margin.detach().cpu().clone())
        return orig(self, t)

    monitor.ValidationMonitor.queue = spy
    try:
        res = fit_gbdt(tr, torch.from_numpy(y[:N_TRAIN]), GBDTParams(n_estimators=8, max_depth=4), device=device,
                       eval_set=(va, torch.from_numpy(y[N_TRAIN:]), None), eval_metric="logloss")
    finally:
        monitor.ValidationMonitor.queue = orig
    assert len(res.trees) == 8 and len(seen) == 8
    m = torch.full((2000,), res.base_margin, dtype=torch.float64)
    for t, snap in zip(res.trees, seen):
        m = m + score_csr(va, ensemble_arrays([t], "value", cmp_less=True))[:, 0]
        assert torch.equal(snap, m)


@pytest.mark.parametrize("device", DEVICES)
def test_validation_value_on_a_threshold_goes_right(device):
    """Generic (non-count) path: training values {-1.5, 0 (absent), 2.5} give the midpoint
    thresholds -0.75 and 1.25; validation values exactly on them follow ``<`` (right), where the
    training rule ``<=`` would send them left."""
    rng = np.random.default_rng(0)
    n = 600
    x = rng.choice([-1.5, 0.0, 2.5], n)
    other = rng.choice([0.0, 1.0], n)
    y = ((x > 0) | ((x < 0) & (other > 0))).astype(np.float32)
    tr = _csr_vc(np.stack([x, other], 1))
    va = _csr_vc(np.array([[-0.75, 1.0], [1.25, 0.0], [-0.75, 0.0], [1.2, 0.0], [-0.8, 1.0]]))
    yva = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0])
    res = fit_gbdt(tr, torch.from_numpy(y), GBDTParams(n_estimators=3, max_depth=2), device=device,
                   eval_set=(va, yva, None), eval_metric="logloss")
    thr = sorted({float(v) for t in res.trees for v, f in zip(t.threshold, t.feature) if f == 0})
    assert -0.75 in thr and 1.25 in thr
    m_less = res.base_margin + score_csr(va, ensemble_arrays(res.trees, "value", cmp_less=True))[:, 0].numpy()
    m_leq = res.base_margin + score_csr(va, ensemble_arrays(res.trees, "value", cmp_less=False))[:, 0].numpy()
    assert not np.array_equal(m_less[:3], m_leq[:3]) and np.array_equal(m_less[3:], m_leq[3:])
    got = res.evals_result["validation"]["logloss"][-1]
    assert abs(got - np_logloss(m_less, yva.numpy())) <= logloss_bound(5)
    assert abs(got - np_logloss(m_leq, yva.numpy())) > 0.01


# ------------------------------------------------------------------------------- 2. + 3. metrics, early stopping
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("metric", METRICS)
def test_history_equals_independent_metrics_without_stopping(device, metric):
    d = Data.get(device)
    res = fit_gbdt(d.tr, d.ytr, PARAMS, device=device, eval_set=(d.va, d.yva, None), eval_metric=metric)
    assert res.deferred is True                              # monitoring keeps the deferred pipeline
    assert _sig(res.trees) == _sig(d.plain.trees)            # all trees kept, training untouched
    hist = res.evals_result["validation"][metric]
    assert len(hist) == ROUNDS
    if metric == "logloss":
        diff = max(abs(a - b) for a, b in zip(hist, d.expected[metric]))
        print(f"logloss {device}: max |history - fsum reference| = {diff:.3e} (bound {logloss_bound(2000):.3e})")
        assert diff <= logloss_bound(2000)
    else:
        assert hist == d.expected[metric]                    # bitwise
    best = 0                                                 # the first round with the best value
    for t in range(1, ROUNDS):
        if (hist[t] > hist[best]) if metric == "auc" else (hist[t] < hist[best]):
            best = t
    assert res.best_iteration == best and res.best_score == hist[best]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("metric", METRICS)
def test_early_stopping_semantics(device, metric):
    d = Data.get(device)
    best, stop = d.best(metric)
    assert best + 1 < ROUNDS and stop == best + PATIENCE       # these inputs do trigger the stop
    res = fit_gbdt(d.tr, d.ytr, PARAMS, device=device, eval_set=(d.va, d.yva, None), eval_metric=metric,
                   early_stopping_rounds=PATIENCE)
    assert res.best_iteration == best
    assert len(res.trees) == best + 1
    assert _sig(res.trees) == _sig(d.plain.trees[:best + 1])
    hist = res.evals_result["validation"][metric]
    assert len(hist) == best + PATIENCE + 1
    if metric == "logloss":
        assert max(abs(a - b) for a, b in zip(hist, d.expected[metric])) <= logloss_bound(2000)
    else:
        assert hist == d.expected[metric][:len(hist)]
    assert res.best_score == hist[best]
    # a strict best: no earlier round ties it
    assert all((h < hist[best]) if metric == "auc" else (h > hist[best]) for h in hist[:best])


def test_weighted_metrics_against_independent_reference():
    d = Data.get("cpu")
    rng = np.random.default_rng(3)
    w = (rng.integers(1, 17, 2000) * 0.25).astype(np.float32)
    p8 = GBDTParams(n_estimators=8, max_depth=4)
    for metric in ("logloss", "error"):
        res = fit_gbdt(d.tr, d.ytr, p8, device="cpu", eval_set=(d.va, d.yva, w), eval_metric=metric)
        assert _sig(res.trees) == _sig(d.plain.trees[:8])        # validation weights do not touch training
        for t, got in enumerate(res.evals_result["validation"][metric]):
            m, yv = d.margins[t], d.y[N_TRAIN:]
            pr = 1.0 / (1.0 + np.exp(-m))
            if metric == "error":
                assert got == float(np.sum(w.astype(np.float64) * ((pr > 0.5) != (yv > 0.5)))) / float(w.sum(dtype=np.float64))
            else:
                terms = [wi * (-math.log(max(1.0 / (1.0 + math.exp(-v)), 1e-16)) if lab > 0.5 else
                               -math.log(max(1.0 - 1.0 / (1.0 + math.exp(-v)), 1e-16)))
                         for v, lab, wi in zip(m.tolist(), yv.tolist(), w.tolist())]
                ws = float(w.sum(dtype=np.float64))
                assert abs(got - math.fsum(terms) / ws) <= logloss_bound(2000, ws, 4.0)


# ------------------------------------------------------------------------------- 4. estimator
def _frame(with_weights=False):
    X, y = _int_features(6000, 11)
    ind = np.zeros(6000, dtype=bool)
    ind[N_TRAIN:] = True
    cols = {"features": _csr_vc(X), "label": y.astype(np.float64), "is_val": ind}
    if with_weights:
        cols["w"] = (np.random.default_rng(3).integers(1, 17, 6000) * 0.25).astype(np.float64)
    return Frame(cols)


EST_KW = dict(features_col="features", label_col="label", n_estimators=ROUNDS, max_depth=4, learning_rate=0.3)


def test_estimator_indicator_column_equals_manual_split(tmp_path):
    d = Data.get("cpu")
    best, _ = d.best("auc")
    model = SparkXGBClassifier(validation_indicator_col="is_val", early_stopping_rounds=PATIENCE, eval_metric="auc",
                               **EST_KW).fit(_frame())
    manual = fit_gbdt(d.tr, d.ytr, PARAMS, device="cpu", eval_set=(d.va, d.yva, None), eval_metric="auc",
                      early_stopping_rounds=PATIENCE)
    assert _sig(model.trees) == _sig(manual.trees) and model.base_margin == manual.base_margin
    assert model.best_iteration == manual.best_iteration == best
    assert model.best_score == manual.best_score and model.evals_result == manual.evals_result
    # the Spark-layout round trip keeps the three attributes
    model.save(tmp_path / "m")
    back = Params.load(tmp_path / "m")
    assert isinstance(back, SparkXGBClassifierModel) and _sig(back.trees) == _sig(model.trees)
    assert (back.best_iteration, back.best_score, back.evals_result) == \
        (model.best_iteration, model.best_score, model.evals_result)
    # and the xgboost JSON carries them as strings, as xgboost writes them
    attrs = model.to_xgboost_json()["learner"]["attributes"]
    assert attrs["best_iteration"] == str(best) and float(attrs["best_score"]) == model.best_score


def test_estimator_weight_column_is_split_with_the_rows():
    d = Data.get("cpu")
    df = _frame(with_weights=True)
    w = np.asarray(df.column("w"), dtype=np.float32)
    model = SparkXGBClassifier(validation_indicator_col="is_val", weight_col="w", eval_metric="logloss",
                               **{**EST_KW, "n_estimators": 6}).fit(df)
    manual = fit_gbdt(d.tr, d.ytr, GBDTParams(n_estimators=6, max_depth=4, learning_rate=0.3), device="cpu",
                      weights=w[:N_TRAIN], eval_set=(d.va, d.yva, w[N_TRAIN:]), eval_metric="logloss")
    assert _sig(model.trees) == _sig(manual.trees) and model.evals_result == manual.evals_result


def test_without_indicator_saved_model_is_byte_identical_to_the_golden_copy(tmp_path, monkeypatch):
    """tests/golden/xgb_no_validation: the files the estimator wrote for this fit before the
    validation parameters existed (fixed uid and timestamp)."""
    monkeypatch.setattr(sf.time, "time", lambda: 1700000000.0)
    X, y = _int_features(6000, 11)
    df = Frame({"features": _csr_vc(X[:N_TRAIN]), "label": y[:N_TRAIN].astype(np.float64)})
    model = SparkXGBClassifier(uid="SparkXGBClassifier_golden", features_col="features", label_col="label",
                               n_estimators=3, max_depth=4, eval_metric="not-a-metric").fit(df)
    assert model.best_iteration is None and model.evals_result == {}
    model.save(tmp_path / "m")
    assert (tmp_path / "m" / "metadata" / "part-00000").read_bytes() == (GOLDEN / "metadata.json").read_bytes()
    assert (tmp_path / "m" / "model" / "part-00000").read_bytes() == (GOLDEN / "model.json").read_bytes()
    assert model.to_xgboost_json()["learner"]["attributes"] == {}


# ------------------------------------------------------------------------------- 6. data parallel, checkpoints
def _rank_fit(rank, world, metric, ck=None, resume=False):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = _int_features(6000, 11)
    lo, hi = shard_range(N_TRAIN, rank, world)
    vlo, vhi = shard_range(6000 - N_TRAIN, rank, world)
    va, yva = _csr_vc(X[N_TRAIN + vlo:N_TRAIN + vhi]), torch.from_numpy(y[N_TRAIN + vlo:N_TRAIN + vhi])
    kw = dict(checkpoint_dir=ck, checkpoint_every=4, resume=resume) if ck else {}
    res = fit_gbdt(_csr_vc(X[lo:hi]), torch.from_numpy(y[lo:hi]), PARAMS, device="cpu", eval_set=(va, yva, None),
                   eval_metric=metric, early_stopping_rounds=PATIENCE, **kw)
    return _sig(res.trees), res.evals_result, res.best_iteration, res.best_score


@pytest.mark.parametrize("metric", ["auc", "logloss"])
def test_data_parallel_history_is_bitwise_world_one(metric):
    single = _rank_fit(0, 1, metric)
    for world in (2, 3):
        outs = spawn(_rank_fit, world, metric, backend="gloo", timeout=300)
        assert all(o == single for o in outs)


def test_num_workers_equals_single_process(monkeypatch):
    monkeypatch.setenv("FDX_DP_MIN_ROWS", "0")
    kw = dict(validation_indicator_col="is_val", early_stopping_rounds=PATIENCE, eval_metric="logloss", **EST_KW)
    single = SparkXGBClassifier(**kw).fit(_frame())
    multi = SparkXGBClassifier(num_workers=2, **kw).fit(_frame())
    assert _sig(multi.trees) == _sig(single.trees)
    assert (multi.best_iteration, multi.best_score, multi.evals_result) == \
        (single.best_iteration, single.best_score, single.evals_result)


def test_killed_fit_resumes_with_the_same_history(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.parallel.checkpoint import EnsembleCheckpointer, InjectedFault

    ref = _rank_fit(0, 1, "auc")
    ck = str(tmp_path / "ck")
    monkeypatch.setenv("FDX_FAULT", "tree:9")
    with pytest.raises(InjectedFault):
        _rank_fit(0, 1, "auc", ck)
    monkeypatch.delenv("FDX_FAULT")
    st = EnsembleCheckpointer(ck).load()
    assert st["trees_done"] == 8 and len(st["evals_result"]["validation"]["auc"]) == 8 and "best_score" in st
    assert _rank_fit(0, 1, "auc", ck, True) == ref
    # a checkpoint without the validation keys resumes only without eval_set
    path = EnsembleCheckpointer(ck).state_path
    old = {k: v for k, v in json.loads(path.read_text()).items()
           if k not in ("evals_result", "best_iteration", "best_score")}
    path.write_text(json.dumps(old))
    with pytest.raises(RuntimeError, match="validation history"):
        _rank_fit(0, 1, "auc", ck, True)


# ------------------------------------------------------------------------------- 7. error cases
def test_error_cases():
    d = Data.get("cpu")
    p3 = GBDTParams(n_estimators=3, max_depth=3)
    ones = torch.ones(2000)
    with pytest.raises(ValueError, match="one class"):
        fit_gbdt(d.tr, d.ytr, p3, device="cpu", eval_set=(d.va, ones, None), eval_metric="auc")
    with pytest.raises(ValueError, match="unknown eval_metric"):
        fit_gbdt(d.tr, d.ytr, p3, device="cpu", eval_set=(d.va, d.yva, None), eval_metric="aucpr")
    with pytest.raises(NotImplementedError):
        fit_gbdt(d.tr, d.ytr, p3, device="cpu", eval_set=(d.va, d.yva, np.ones(2000, np.float32)), eval_metric="auc")
    empty = VectorColumn(10, torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                         torch.zeros(0, dtype=torch.float64))
    with pytest.raises(ValueError, match="empty"):
        fit_gbdt(d.tr, d.ytr, p3, device="cpu", eval_set=(empty, torch.zeros(0), None), eval_metric="logloss")
    df = _frame(with_weights=True)
    with pytest.raises(NotImplementedError):
        SparkXGBClassifier(validation_indicator_col="is_val", weight_col="w", eval_metric="auc", **EST_KW).fit(df)
    with pytest.raises(ValueError, match="unknown eval_metric"):
        SparkXGBClassifier(validation_indicator_col="is_val", eval_metric="aucpr", **EST_KW).fit(df)
    # without validation the metric stays inert: unknown values are accepted
    assert len(fit_gbdt(d.tr, d.ytr, p3, device="cpu", eval_metric="aucpr").trees) == 3


# ------------------------------------------------------------------------------- GPU: the whole fit
def _device_fits(rank=0, world=1):
    X, y = _int_features(6000, 11)        # (only the inputs: a rank process runs no host fit)
    tr, ytr = _csr_vc(X[:N_TRAIN]), torch.from_numpy(y[:N_TRAIN])
    va, yva = _csr_vc(X[N_TRAIN:]), torch.from_numpy(y[N_TRAIN:])
    out = {}
    for metric in METRICS:
        res = fit_gbdt(tr, ytr, PARAMS, device="cuda:0", eval_set=(va, yva, None), eval_metric=metric,
                       early_stopping_rounds=PATIENCE)
        out[metric] = (_sig(res.trees), res.evals_result["validation"][metric], res.best_iteration, res.deferred)
    return out


_HOST_FITS: dict = {}


def _host_fit(metric):
    if metric not in _HOST_FITS:
        d = Data.get("cpu")
        _HOST_FITS[metric] = fit_gbdt(d.tr, d.ytr, PARAMS, device="cpu", eval_set=(d.va, d.yva, None),
                                      eval_metric=metric, early_stopping_rounds=PATIENCE)
    return _HOST_FITS[metric]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "forced_collectives", "no_rowhist"])
def test_gpu_fit_equals_host_fit(mode, monkeypatch):
    """The device fit stops at the host fit's round with the host's trees; auc / error histories
    are bitwise the host's, logloss within 2 * 2^-k + 1e-13 (one rounding flip per row at most
    plus the libm term difference). Also on the RCCL path at world 1 (one rank process: the
    collectives need a process group) and with the CSC histogram passes instead of the row-group
    engine."""
    if mode == "forced_collectives":
        monkeypatch.setenv("FDX_FORCE_COLLECTIVES", "1")
        got, = spawn(_device_fits, 1, backend="nccl", timeout=300)
    else:
        if mode == "no_rowhist":
            from fraud_detection_spark_kafka_llm_amd.models import grower

            monkeypatch.setattr(grower, "ROWHIST", False)
        got = _device_fits()
    k = int(native.lib().eval_sum_kexp(2000, 1.0))
    for metric in METRICS:
        host = _host_fit(metric)
        trees, hist, best, deferred = got[metric]
        assert trees == _sig(host.trees) and best == host.best_iteration and deferred
        want = host.evals_result["validation"][metric]
        if metric == "logloss":
            diff = max(abs(a - b) for a, b in zip(hist, want))
            print(f"logloss {mode}: max |device - host| = {diff:.3e} (bound {2 * 2.0 ** -k + 1e-13:.3e})")
            assert len(hist) == len(want) and diff <= 2 * 2.0 ** -k + 1e-13
        else:
            assert hist == want
