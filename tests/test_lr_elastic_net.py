"""Elastic-net logistic regression (OWL-QN on csrc/lr_kernels.hip / lr_cpu.cpp): the optimum against
a NumPy FISTA reference and a KKT certificate computed from the returned coefficients alone, the
four kernels and their host twins against exact NumPy references and a derivable summation bound,
the routes that must not change, and the model through the pipeline, the Spark layout, the
streaming scorer, data parallelism and the sanitized self-test."""
import functools
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd import _build
from fraud_detection_spark_kafka_llm_amd.data import synth
from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
from fraud_detection_spark_kafka_llm_amd.ml import (IDF, Frame, HashingTF, LogisticRegression, Pipeline, PipelineModel,
                                                     StopWordsRemover, TextColumn, TokenColumn, Tokenizer)
from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.stopwords import ENGLISH
from fraud_detection_spark_kafka_llm_amd.models import lr as LR
from fraud_detection_spark_kafka_llm_amd.ops import native
from fraud_detection_spark_kafka_llm_amd.ops import oracle as O
from fraud_detection_spark_kafka_llm_amd.ops import sparse as S
from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

C = native.lib()
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
CASES = [(0.02, 1.0), (0.05, 0.3)]          # (regParam, elasticNetParam)
# relative error of lr_forward's per-row terms against the NumPy fp64 formula: 4 x the largest error
# measured on the MI355X over these cases (4.121e-16, profiles/r12/lr_elastic_net.md), never above 1e-13
ROW_TERM_RTOL = min(4 * 4.121e-16, 1e-13)


def test_limits_are_exported():
    lim = S.lr_limits()
    assert set(lim) >= {"rows_per_partial", "reduce_block", "block"}
    assert lim["rows_per_partial"] * 64 == lim["block"] and lim["reduce_block"] == 256


# ------------------------------------------------------------------------------- corpus and reference
@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(11)
    X = (rng.random((800, 150)) < 0.08) * rng.random((800, 150)) * 4
    y = (X[:, :12].sum(1) + rng.normal(0, 0.3, 800) > 1.0).astype(np.float64)
    return X, y


def feature_scale(X):
    std = X.std(0, ddof=1)
    return np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)


def smooth_grad(Z, y, theta):
    """Gradient of the mean log-loss over the columns of ``Z`` (the last one is the intercept's ones)."""
    m = Z @ theta
    return Z.T @ (1.0 / (1.0 + np.exp(-m)) - y) / len(y)


def objective(Z, y, theta, l1, l2):
    m = Z @ theta
    beta = theta[:-1]
    return float(np.mean(np.maximum(m, 0) - m * y + np.log1p(np.exp(-np.abs(m)))) + 0.5 * l2 * beta @ beta
                 + l1 * np.abs(beta).sum())


@functools.lru_cache(maxsize=None)
def fista(reg, alpha, iters=4000):
    """FISTA with restart on the standardised problem, in plain NumPy: (theta, objective, Z, scale)."""
    X, y = corpus()
    l1, l2 = reg * alpha, reg * (1.0 - alpha)
    n, F = X.shape
    sc = feature_scale(X)
    Z = np.hstack([X * sc, np.ones((n, 1))])
    lip = 0.25 * np.linalg.norm(Z, 2) ** 2 / n + l2
    th, v, tk = np.zeros(F + 1), np.zeros(F + 1), 1.0
    for _ in range(iters):
        g = smooth_grad(Z, y, v)
        g[:F] += l2 * v[:F]
        u = v - g / lip
        new = u.copy()
        new[:F] = np.sign(u[:F]) * np.maximum(np.abs(u[:F]) - l1 / lip, 0.0)
        if np.dot(v - new, new - th) > 0:
            tk = 1.0
        tn = (1.0 + math.sqrt(1.0 + 4.0 * tk * tk)) / 2.0
        v = new + (tk - 1.0) / tn * (new - th)
        th, tk = new, tn
    return th, objective(Z, y, th, l1, l2), Z, sc


def kkt_residual(Z, y, theta, l1, l2):
    """Largest violation of the optimality conditions over coefficients and intercept."""
    g = smooth_grad(Z, y, theta)
    beta, gb = theta[:-1], g[:-1]
    nz = beta != 0
    worst = abs(g[-1])
    if nz.any():
        worst = max(worst, np.abs(gb[nz] + l2 * beta[nz] + l1 * np.sign(beta[nz])).max())
    if (~nz).any():
        worst = max(worst, (np.abs(gb[~nz]) - l1).max())
    return float(worst)


@functools.lru_cache(maxsize=None)
def fitted(reg, alpha, device, standardization=True):
    X, y = corpus()
    vc = VectorColumn(X.shape[1], dense=torch.from_numpy(X))
    return LR.train_logistic_regression(vc, y, max_iter=500, tol=1e-12, reg_param=reg, elastic_net=alpha,
                                        standardization=standardization, device=device)


def test_reference_is_converged():
    for reg, alpha in CASES:
        th, _, Z, _ = fista(reg, alpha)
        assert kkt_residual(Z, corpus()[1], th, reg * alpha, reg * (1 - alpha)) < 1e-12
    assert [int((fista(*c)[0][:-1] != 0).sum()) for c in CASES] == [13, 26]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reg,alpha", CASES)
def test_optimum_matches_reference(reg, alpha, device):
    th, ref_obj, Z, sc = fista(reg, alpha)
    coef, b, hist = fitted(reg, alpha, device)
    y = corpus()[1]
    F = coef.size
    theta = np.append(np.where(sc > 0, coef / np.where(sc > 0, sc, 1.0), 0.0), b)
    obj = objective(Z, y, theta, reg * alpha, reg * (1 - alpha))
    diff = np.abs(np.append(coef, b) - np.append(th[:F] * sc, th[F])).max()
    print(f"reg={reg} alpha={alpha} {device}: objective gap {obj - ref_obj:.3e}, history gap {hist[-1] - ref_obj:.3e}, "
          f"max |coef - ref| {diff:.3e}, non-zeros {int((coef != 0).sum())}, evaluations {len(hist)}")
    assert np.array_equal(coef != 0, th[:F] != 0)
    assert np.all(coef[th[:F] == 0] == 0.0)                   # exact zeros, not small numbers
    assert obj <= ref_obj + 1e-10 and hist[-1] <= ref_obj + 1e-10
    assert diff <= 1e-4
    assert all(a >= b_ for a, b_ in zip(hist, hist[1:]))      # the full objective never increases


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reg,alpha", CASES)
def test_kkt_certificate(reg, alpha, device):
    _, _, Z, sc = fista(reg, alpha)
    coef, b, _ = fitted(reg, alpha, device)
    theta = np.append(np.where(sc > 0, coef / np.where(sc > 0, sc, 1.0), 0.0), b)
    l1, l2 = reg * alpha, reg * (1 - alpha)
    g = smooth_grad(Z, corpus()[1], theta)
    beta, gb = theta[:-1], g[:-1]
    nz = beta != 0
    res = kkt_residual(Z, corpus()[1], theta, l1, l2)
    print(f"reg={reg} alpha={alpha} {device}: KKT residual {res:.3e}")
    assert np.all(np.abs(gb[nz] + l2 * beta[nz] + l1 * np.sign(beta[nz])) <= 1e-5)
    assert np.all(np.abs(gb[~nz]) <= l1 + 1e-5)
    assert abs(g[-1]) <= 1e-5


# ------------------------------------------------------------------------------- routes
def _determinism_corpus():
    rng = np.random.default_rng(11)
    n, F = 3000, 400
    dense = (rng.random((n, F)) < 0.05) * rng.random((n, F)) * 4
    y = (dense[:, :20].sum(1) + rng.normal(0, 0.3, n) > 1.0).astype(float)
    return VectorColumn(F, dense=torch.from_numpy(dense)), y


def test_other_routes_never_reach_owlqn(monkeypatch):
    """regParam > 0 with elasticNetParam = 0, and regParam = 0 with any elasticNetParam, run the L-BFGS
    body: the new trainer is not entered and the results are bitwise those of the plain calls."""
    def boom(*a, **k):
        raise AssertionError("the OWL-QN route was taken")

    vc, y = _determinism_corpus()
    plain_l2 = LR.train_logistic_regression(vc, y, max_iter=40, reg_param=0.01, device="cpu")
    plain_0 = LR.train_logistic_regression(vc, y, max_iter=40, device="cpu")
    monkeypatch.setattr(LR, "_train_owlqn", boom)
    runs = [(plain_l2, dict(reg_param=0.01, elastic_net=0.0)), (plain_0, dict(reg_param=0.0, elastic_net=0.5)),
            (plain_0, dict(reg_param=0.0, elastic_net=1.0))]
    for want, kw in runs:
        got = LR.train_logistic_regression(vc, y, max_iter=40, device="cpu", **kw)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    with pytest.raises(AssertionError, match="OWL-QN route"):
        LR.train_logistic_regression(vc, y, max_iter=2, reg_param=0.01, elastic_net=0.5, device="cpu")


@pytest.mark.parametrize("kw", [dict(elastic_net=1.5, reg_param=0.1), dict(elastic_net=-0.1, reg_param=0.1),
                                dict(reg_param=-1.0), dict(elastic_net=1.5)])
def test_invalid_parameters_raise(kw):
    X, y = corpus()
    with pytest.raises(ValueError):
        LR.train_logistic_regression(VectorColumn(X.shape[1], dense=torch.from_numpy(X)), y, device="cpu", **kw)


def test_multinomial_stays_unsupported():
    X, y = corpus()
    frame = Frame({"features": VectorColumn(X.shape[1], dense=torch.from_numpy(X)), "label": y})
    with pytest.raises(NotImplementedError):
        LogisticRegression(family="multinomial", regParam=0.02, elasticNetParam=1.0).fit(frame)


# ------------------------------------------------------------------------------- standardisation
def test_without_standardisation_kkt_holds_on_raw_features():
    X, y = corpus()
    reg, alpha = 0.02, 1.0
    coef, b, _ = fitted(reg, alpha, "cpu", standardization=False)
    Z = np.hstack([X, np.ones((len(y), 1))])
    theta = np.append(coef, b)
    g = smooth_grad(Z, y, theta)
    nz = coef != 0
    assert 0 < nz.sum() < coef.size
    assert np.all(np.abs(g[:-1][nz] + reg * alpha * np.sign(coef[nz])) <= 1e-5)      # one lambda_1 for every feature
    assert np.all(np.abs(g[:-1][~nz]) <= reg * alpha + 1e-5)
    assert abs(g[-1]) <= 1e-5


def test_constant_feature_gets_coefficient_zero():
    X, y = corpus()
    Xc = np.hstack([X, np.full((len(y), 1), 2.5)])
    coef, b, _ = LR.train_logistic_regression(VectorColumn(Xc.shape[1], dense=torch.from_numpy(Xc)), y, max_iter=500,
                                              tol=1e-12, reg_param=0.02, elastic_net=1.0, device="cpu")
    assert coef[-1] == 0.0
    base = fitted(0.02, 1.0, "cpu")
    assert np.array_equal(coef[:-1] != 0, base[0] != 0)
    np.testing.assert_allclose(coef[:-1], base[0], atol=1e-4)


# ------------------------------------------------------------------------------- lr_forward
ROW_LENGTHS = (0, 1, 63, 64, 65, 129)
FORCED = (40.0, -40.0, 800.0, -800.0)


@functools.lru_cache(maxsize=None)
def forward_case(rows):
    """Rows of 0, 1, 63, 64, 65, 129 entries; the empty rows have margin b = 0, the one-entry rows
    hit coefficients of +-40 and +-800, every other margin stays small (|m| < 5), so sigma(m) - y
    loses no more than a few bits to cancellation and a relative bound on r is meaningful."""
    rng = np.random.default_rng(rows)
    F = 130 + len(FORCED)
    xs = np.concatenate([rng.uniform(-0.4, 0.4, 130), FORCED])
    indptr, idx, val = [0], [], []
    for r in range(rows):
        ln = ROW_LENGTHS[r % len(ROW_LENGTHS)]
        if ln == 1:
            idx.append(130 + (r // len(ROW_LENGTHS)) % len(FORCED))
            val.append(1.0)
        else:
            idx.extend(range(ln))
            val.extend(rng.uniform(-0.5, 0.5, ln))
        indptr.append(len(idx))
    mix = np.arange(rows) + np.arange(rows) // len(ROW_LENGTHS)      # every (length, label, weight) combination
    y = (mix % 2).astype(np.float64)
    w = np.asarray([0.0, 0.5, 3.0])[mix % 3]
    return (np.asarray(indptr, np.int64), np.asarray(idx, np.int32), np.asarray(val, np.float64), xs, y, w, F)


def fsum_bound_ok(total, terms):
    """|total - sum(terms)| <= (n - 1) 2^-53 sum|terms|: any summation order of n terms obeys it
    to first order; math.fsum gives the exact sum, correctly rounded."""
    terms = np.asarray(terms, np.float64)
    return abs(total - math.fsum(terms)) <= max(len(terms) - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(terms))


def rel_err(got, want):
    return float((np.abs(got - want) / np.maximum(np.abs(want), 2.0 ** -1022)).max())


def partials_by_hand(terms, per):
    """One partial per ``per`` rows, the rows added in order from 0.0 (padding adds +0.0 at the end)."""
    P = (len(terms) + per - 1) // per
    pad = np.zeros(P * per)
    pad[:len(terms)] = terms
    pad = pad.reshape(P, per)
    acc = np.zeros(P)
    for k in range(per):
        acc = acc + pad[:, k]
    return acc


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("val_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("rows", [3, 4, 5, 1025])
def test_lr_forward(rows, val_dtype, device):
    indptr, idx, val, xs, y, w, F = forward_case(rows)
    t = [torch.from_numpy(a).to(device) for a in (indptr, idx, val, xs, y, w)]
    t[2] = t[2].to(val_dtype)
    per = S.lr_limits()["rows_per_partial"]
    for b in (0.0, 0.25):
        bt = torch.tensor([b], dtype=torch.float64, device=device)
        r, sums, loss_row, margin = S.lr_forward(t[0], t[1], t[2], t[3], bt, t[4], t[5], want_rows=True)
        assert torch.equal(margin, S.spmv(t[0], t[1], t[2], t[3]) + b)              # bitwise, same device
        m = margin.cpu().numpy()
        assert np.isfinite(m).all()
        if b == 0.0:
            have = set(m.tolist())
            assert 0.0 in have and (rows < 1025 or have >= {40.0, -40.0, 800.0, -800.0})
        e = np.exp(-np.abs(m))
        want_loss = np.maximum(m, 0) - m * y + np.log1p(e)
        want_r = w * (np.where(m >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) - y)
        got_loss, got_r = loss_row.cpu().numpy(), r.cpu().numpy()
        assert np.isfinite(got_loss).all() and np.isfinite(got_r).all()
        print(f"rows={rows} b={b} {device} {val_dtype}: rel err loss {rel_err(got_loss, want_loss):.3e} "
              f"r {rel_err(got_r, want_r):.3e}")
        assert rel_err(got_loss, want_loss) <= ROW_TERM_RTOL and rel_err(got_r, want_r) <= ROW_TERM_RTOL
        s = sums.cpu().numpy()
        assert fsum_bound_ok(s[0], w * got_loss) and fsum_bound_ok(s[1], got_r)
        # repeatable, and the sums of the host twin's reduction fed the same per-row outputs
        again = S.lr_forward(t[0], t[1], t[2], t[3], bt, t[4], t[5])
        assert torch.equal(again[1], sums) and torch.equal(again[0], r)
        by_hand = np.stack([partials_by_hand(w * got_loss, per), partials_by_hand(got_r, per)])
        host = S.lr_reduce(torch.from_numpy(by_hand))
        assert np.array_equal(host.numpy(), s)


def test_lr_reduce_order_is_strided_then_a_tree():
    """Lane t adds partials t, t + 256, ... in ascending order, then a tree over the 256 lanes."""
    rng = np.random.default_rng(5)
    width = S.lr_limits()["reduce_block"]
    for P in (0, 1, 255, 256, 257, 1000):
        p = rng.standard_normal((2, P)) * 10.0 ** rng.integers(-8, 8, (2, P))
        lanes = np.zeros((2, width))
        for i in range(P):
            lanes[:, i % width] = lanes[:, i % width] + p[:, i]
        o = width // 2
        while o:
            lanes[:, :o] = lanes[:, :o] + lanes[:, o:2 * o]
            o //= 2
        assert np.array_equal(S.lr_reduce(torch.from_numpy(p)).numpy(), lanes[:, 0])


# ------------------------------------------------------------------------------- parameter passes
PARAM_SIZES = [1, 2, 255, 256, 257, 65537]


@functools.lru_cache(maxsize=None)
def param_case(n):
    """x with exact zeros, directions that flip signs under a unit step, pg with exact zeros."""
    rng = np.random.default_rng(n)
    kind = np.arange(n) % 5
    x = np.where(kind == 0, 0.0, rng.uniform(-1, 1, n))
    d = np.where(kind == 1, -4.0 * x, rng.uniform(-0.5, 0.5, n))
    pg = np.where(kind == 2, 0.0, rng.uniform(-0.5, 0.5, n))
    xi = np.where(x != 0, np.sign(x), np.sign(-pg))
    scale = np.where(np.arange(n - 1) % 7 == 3, 0.0, rng.uniform(0.5, 1.5, n - 1))
    parts = rng.uniform(-4, 4, n + 1)
    return x, d, xi, pg, scale, parts


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", PARAM_SIZES)
def test_lr_owlqn_step(n, device):
    x, d, xi, pg, scale, _ = param_case(n)
    F = n - 1
    dev = [torch.from_numpy(a).to(device) for a in (x, d, xi, pg, scale)]
    for t in (1.0, 2.0 ** -7):
        x_new, xs_new, sums = S.lr_owlqn_step(*dev, t)
        v = x + t * d
        want = np.where(((xi > 0) & (v > 0)) | ((xi < 0) & (v < 0)), v, 0.0)
        want[F] = v[F]                                             # the intercept slot is never projected
        got = x_new.cpu().numpy()
        assert got.tobytes() == want.tobytes()                     # bitwise, zeros are +0.0
        assert xs_new.cpu().numpy().tobytes() == (scale * want[:F]).tobytes()
        if n > 2 and t == 1.0:
            assert np.any((want[:F] == 0) & (x[:F] != 0))          # a coefficient left its orthant
        s = sums.cpu().numpy()
        assert fsum_bound_ok(s[0], np.abs(want[:F])) and fsum_bound_ok(s[1], want[:F] * want[:F])
        assert fsum_bound_ok(s[2], pg * (want - x))
        host = S.lr_owlqn_step(*(a.cpu() for a in dev), t)
        assert torch.equal(host[2], sums.cpu()) and torch.equal(host[0], x_new.cpu())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", PARAM_SIZES)
def test_lr_pseudo_grad(n, device):
    x, _, _, _, scale, parts = param_case(n)
    F = n - 1
    W, l1, l2 = 37.0, 0.125, 0.25
    beta, xtr = x[:F], parts[2:]
    for fit in (True, False):
        g, pg, xi, nn = S.lr_pseudo_grad(torch.from_numpy(parts).to(device), torch.from_numpy(scale).to(device),
                                         torch.from_numpy(x).to(device), W, l1, l2, fit)
        wg = scale * xtr / W + l2 * beta
        up, dn = wg + l1, wg - l1
        wpg = np.where(beta > 0, up, np.where(beta < 0, dn, np.where(up < 0, up, np.where(dn > 0, dn, 0.0))))
        wxi = np.where(beta > 0, 1.0, np.where(beta < 0, -1.0, np.where(wpg < 0, 1.0, np.where(wpg > 0, -1.0, 0.0))))
        gb = parts[1] / W if fit else 0.0
        wg, wpg, wxi = np.append(wg, gb), np.append(wpg, gb), np.append(wxi, 0.0)
        assert g.cpu().numpy().tobytes() == wg.tobytes()
        assert pg.cpu().numpy().tobytes() == wpg.tobytes()
        assert xi.cpu().numpy().tobytes() == wxi.tobytes()
        if n > 5:
            assert np.any((beta == 0) & (wpg[:F] == 0)) and np.any((beta == 0) & (wpg[:F] != 0))
        assert fsum_bound_ok(float(nn[0]), wpg * wpg)
        host = S.lr_pseudo_grad(torch.from_numpy(parts), torch.from_numpy(scale), torch.from_numpy(x), W, l1, l2, fit)
        assert torch.equal(host[3], nn.cpu())


def test_parameter_passes_reject_misaligned_views():
    x, d, xi, pg, scale, _ = param_case(257)
    t = [torch.from_numpy(np.concatenate([[0.0], a]))[1:] for a in (x, d, xi, pg, scale)]
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        S.lr_owlqn_step(*t, 1.0)


# ------------------------------------------------------------------------------- through the stack
def _dialogue_frame(n=400, seed=21):
    pt, y = synth.generate(synth.SynthConfig(n=n, seed=seed))
    raw = TextColumn(pt.strings())
    return Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})


def _stages():
    return [Tokenizer(inputCol="clean_text", outputCol="words"),
            StopWordsRemover(inputCol="words", outputCol="filtered_words"),
            HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
            IDF(inputCol="raw_features", outputCol="features"),
            LogisticRegression(featuresCol="features", labelCol="labels", regParam=0.02, elasticNetParam=1.0, maxIter=50)]


def _staged(model, frame):
    """Stage by stage over materialised tokens: every stage runs its host path."""
    toks = [O.remove_stopwords(O.tokenize(s), ENGLISH) for s in frame.column("clean_text").strings]
    out = frame.withColumn("filtered_words", TokenColumn(frame.column("clean_text"), tokens=toks))
    for s in model.stages[2:]:
        out = s.transform(out)
    return out


@pytest.mark.parametrize("device", DEVICES)
def test_pipeline_spark_layout_and_contributions(device, tmp_path, monkeypatch):
    monkeypatch.setenv("FDX_DEVICE", device)
    df = _dialogue_frame()
    model = Pipeline(stages=_stages()).fit(df)
    lr = model.stages[-1]
    nnz = int((lr.coefficients != 0).sum())
    assert 0 < nnz < 4096 // 4 and len(lr.objectiveHistory) > 1
    fused, staged = model.transform(df), _staged(model, df)
    for col in ("rawPrediction", "probability", "prediction"):
        assert torch.equal(torch.as_tensor(fused.column(col)).cpu(), torch.as_tensor(staged.column(col)).cpu()), col
    acc = float((torch.as_tensor(fused.column("prediction")).cpu().numpy() == df.column("labels")).mean())
    assert acc > 0.9
    # Spark layout: a sparse coefficientMatrix that stores exactly the non-zero coefficients
    path = tmp_path / "m"
    model.write().overwrite().save(str(path))
    stage_dir = path / "stages" / f"4_{lr.uid}"
    row = sf.read_data_parquet(stage_dir).to_pylist()[0]
    assert row["coefficientMatrix"]["type"] == 0 and len(row["coefficientMatrix"]["values"]) == nnz
    md = json.loads((stage_dir / "metadata" / "part-00000").read_text().splitlines()[0])
    assert md["paramMap"]["elasticNetParam"] == 1.0 and md["paramMap"]["regParam"] == 0.02
    again = PipelineModel.load(str(path))
    assert again.stages[-1].coefficients.tobytes() == lr.coefficients.tobytes()
    assert again.stages[-1].intercept == lr.intercept
    out = again.transform(df)
    assert torch.equal(torch.as_tensor(out.column("rawPrediction")).cpu(), torch.as_tensor(fused.column("rawPrediction")).cpu())
    # contributions: a row sums to its class-1 raw score
    phi = lr.contributions(fused)
    ip, _, v = (a.cpu().numpy() for a in phi.csr())
    raw1 = torch.as_tensor(fused.column("rawPrediction")).cpu().numpy()[:, 1]
    for r in range(0, len(raw1), 7):
        seg = v[ip[r]:ip[r + 1]]
        assert seg.sum() == pytest.approx(raw1[r], abs=1e-12 * (1 + np.abs(seg).sum()))
    # streaming scorer over the compiled pipeline
    from fraud_detection_spark_kafka_llm_amd.stream.gpu_worker import GpuScorer, HostScorer
    from fraud_detection_spark_kafka_llm_amd.stream.ring import PinnedRing

    fp = model.compile(device)
    docs = list(df.column("dialogue").strings)[:128]
    ring = PinnedRing(slots=1, max_docs=128, max_bytes=1 << 20)
    ring.slots[0].fill(docs)
    args = (fp.spec(True), fp.idf.idf, fp.model.scorer())
    scorer = HostScorer(*args, max_docs=128, max_bytes=1 << 20) if device == "cpu" else \
        GpuScorer(*args, device, max_docs=128, max_bytes=1 << 20)
    assert torch.equal(torch.from_numpy(scorer.score_packed(ring.slots[0])), fp.run(docs, clean=True).raw.cpu())


# ------------------------------------------------------------------------------- data parallel
def _dp_fit(rank, world, reg, alpha):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = corpus()
    lo, hi = shard_range(len(y), rank, world)
    vc = VectorColumn(X.shape[1], dense=torch.from_numpy(X[lo:hi]))
    coef, b, hist = LR.train_logistic_regression(vc, y[lo:hi], max_iter=500, tol=1e-12, reg_param=reg,
                                                 elastic_net=alpha, device="cpu")
    return coef.tolist(), b, len(hist)


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_equals_single_process(world):
    reg, alpha = CASES[0]
    single = fitted(reg, alpha, "cpu")
    outs = spawn(_dp_fit, world, reg, alpha, backend="gloo")
    assert all(o == outs[0] for o in outs)                         # identical on every rank
    coef = np.asarray(outs[0][0])
    print(f"world {world}: max |coef - single| {np.abs(coef - single[0]).max():.3e}")
    assert np.array_equal(coef != 0, single[0] != 0)
    np.testing.assert_allclose(coef, single[0], rtol=1e-6, atol=1e-8)
    assert outs[0][1] == pytest.approx(single[1], rel=1e-6)


# ------------------------------------------------------------------------------- repeatability
@pytest.mark.parametrize("device", DEVICES)
def test_fit_is_bitwise_repeatable(device):
    vc, y = _determinism_corpus()
    a, b = (LR.train_logistic_regression(vc, y, max_iter=40, reg_param=0.01, elastic_net=0.5, device=device)
            for _ in range(2))
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]
    assert 0 < (a[0] != 0).sum() < a[0].size


# ------------------------------------------------------------------------------- sanitizer
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="needs hipcc")
def test_lr_host_twins_clean_under_asan_ubsan():
    exe = _build.build_selftest("lr", sanitize=True)
    res = subprocess.run([str(exe)], env={**os.environ, **_build.SELFTEST_ENV}, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "lr selftest ok" in res.stdout
    assert "runtime error" not in res.stderr      # UBSan diagnostics
