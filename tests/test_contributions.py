"""Per-dialogue feature contributions (exact path-dependent TreeSHAP).

The oracle is independent of the path formulation: brute-force Shapley values over a tree's
distinct features, with ``v(S)`` the recursive conditional expectation (follow ``x`` at nodes whose
feature is in ``S``, average the children by cover otherwise). Tolerance against it:
``|delta| <= 1e-10 * V`` with ``V = sum over paths of |leaf value x tree weight|`` -- every term is
bounded by its ``|v|`` and fp64 accumulation of n <= ~1e4 terms errs by <= n * eps * V ~ 1e-12 * V,
which leaves a margin of ~100x. Device results are compared with the host twin bitwise.
"""
import itertools
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd import _build
from fraud_detection_spark_kafka_llm_amd.data import synth
from fraud_detection_spark_kafka_llm_amd.ml import (IDF, DecisionTreeClassifier, Frame, HashingTF,
                                                     LogisticRegressionModel, Pipeline, RandomForestClassifier,
                                                     StopWordsRemover, TextColumn, Tokenizer)
from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import Tree, ensemble_arrays, ensemble_paths
from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier, SparkXGBClassifierModel
from fraud_detection_spark_kafka_llm_amd.ops import oracle as text_oracle
from fraud_detection_spark_kafka_llm_amd.ops.sparse import contrib_limits, score_csr, tree_contributions
from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM

REL_TOL = 1e-10
VALUES = (0.25, 0.5, 1.0, 2.0, 3.0)     # thresholds and row values share this pool (exact in float32)
SIZE = 4096                              # feature space of the hand-made ensembles


# ------------------------------------------------------------------------------- tree builders
def mk_tree(feature, thr, left, right, stats) -> Tree:
    n = len(feature)
    return Tree(np.asarray(feature, np.int32), np.asarray(thr, np.float64), np.asarray(left, np.int32),
                np.asarray(right, np.int32), np.asarray(stats, np.float64).reshape(n, -1), np.zeros(n), np.zeros(n),
                np.zeros(n, np.int64), np.zeros(n), 0)


def random_tree(rng, depth: int, feats, K: int) -> Tree:
    """Random tree of depth <= ``depth``. K = 1: stats = (leaf value, cover); K = 2: class counts.
    An internal node's stats are the sum of its children's (so its cover is)."""
    feature, thr, left, right, stats = [], [], [], [], []

    def grow(d):
        i = len(feature)
        for a in (feature, thr, left, right, stats):
            a.append(None)
        if d == 0 or (d < depth and rng.random() < 0.25):
            feature[i], thr[i], left[i], right[i] = -1, 0.0, -1, -1
            stats[i] = [float(rng.normal()), float(rng.integers(1, 9))] if K == 1 else \
                [float(rng.integers(0, 6)), float(rng.integers(1, 6))]
            return i
        feature[i], thr[i] = int(rng.choice(feats)), float(rng.choice(VALUES))
        left[i], right[i] = grow(d - 1), grow(d - 1)
        s = np.asarray(stats[left[i]]) + np.asarray(stats[right[i]])
        stats[i] = [0.0, s[1]] if K == 1 else list(s)
        return i

    grow(depth)
    return mk_tree(feature, thr, left, right, stats)


def stump(f, t, lv, rv, lc=3.0, rc=5.0) -> Tree:
    return mk_tree([f, -1, -1], [t, 0, 0], [1, -1, -1], [2, -1, -1], [[0, lc + rc], [lv, lc], [rv, rc]])


def tri(f, g, t=1.0) -> Tree:
    """Root on ``f`` with a leaf on the left and a split on ``g`` on the right: three paths through ``f``."""
    return mk_tree([f, -1, g, -1, -1], [t, 0, 0.5, 0, 0], [1, -1, 3, -1, -1], [2, -1, 4, -1, -1],
                   [[0, 9], [0.5, 4], [0, 5], [-1.0, 2], [0.75, 3]])


def leaf_only(v) -> Tree:
    return mk_tree([-1], [0], [-1], [-1], [[v, 4.0]])


def chain(nfeat: int, first: int = 0) -> Tree:
    """A right-going chain over ``nfeat`` distinct features (``nfeat + 1`` leaves)."""
    n = 2 * nfeat + 1
    feature, left, right = [-1] * n, [-1] * n, [-1] * n
    thr, stats = [0.0] * n, [[0.0, 0.0]] * n
    for d in range(nfeat):
        feature[2 * d], thr[2 * d], left[2 * d], right[2 * d] = first + d, 0.5, 2 * d + 1, 2 * d + 2
        stats[2 * d] = [0.0, float(2 + nfeat - d)]
        stats[2 * d + 1] = [math.sin(d + 1.0), 1.0]
    stats[2 * nfeat] = [1.5, 2.0]
    return mk_tree(feature, thr, left, right, stats)


class Ens:
    def __init__(self, trees, payload="value", weights=None, cmp_less=True):
        self.trees, self.payload, self.weights, self.cmp_less = trees, payload, weights, cmp_less
        self.K = 1 if payload == "value" else 2

    def paths(self, output=None):
        return ensemble_paths(self.trees, self.payload, self.weights, self.cmp_less, output)

    def arrays(self):
        return ensemble_arrays(self.trees, self.payload, self.weights, self.cmp_less)


def hand_ensembles() -> dict:
    rng = np.random.default_rng(7)
    feats = [3, 17, 40, 41, 900, 2047, 4000]
    same = mk_tree([5, 5, 5, -1, -1, -1, -1], [2.0, 1.0, 0.5, 0, 0, 0, 0], [1, 2, 3, -1, -1, -1, -1],
                   [6, 5, 4, -1, -1, -1, -1], [[0, 12], [0, 9], [0, 5], [1.0, 2], [-0.5, 3], [2.0, 4], [0.25, 3]])
    return {
        "random_value_lt": Ens([random_tree(rng, 3, feats, 1) for _ in range(6)], "value", None, True),
        "random_value_le": Ens([random_tree(rng, 3, feats, 1) for _ in range(6)], "value", None, False),
        "one_feature_thrice_lt": Ens([same], "value", None, True),
        "one_feature_thrice_le": Ens([same], "value", None, False),
        "single_leaf": Ens([leaf_only(0.75)], "value", None, True),
        "leaf_and_trees": Ens([leaf_only(-0.5), random_tree(rng, 2, feats, 1), leaf_only(2.0)], "value", None, True),
        "normalized_weighted": Ens([random_tree(rng, 3, feats, 2) for _ in range(5)], "normalized",
                                   np.array([0.5, 2.0, 1.0, 0.25, 3.0]), False),
        "counts": Ens([random_tree(rng, 3, feats, 2)], "counts", None, False),
    }


HAND = hand_ensembles()


def rows_with_nnz(nnzs, must_have=(), seed=0, dtype=torch.float64) -> VectorColumn:
    """One row per entry of ``nnzs``: that many distinct features of [0, SIZE), the first ones drawn
    from ``must_have`` (features the model uses), values from the threshold pool."""
    rng = np.random.default_rng(seed)
    ptr, idx, val = [0], [], []
    for m in nnzs:
        own = list(rng.permutation(np.asarray(must_have, dtype=np.int64))[:m]) if len(must_have) else []
        rest = np.setdiff1d(np.arange(SIZE), own)
        ids = np.sort(np.concatenate([own, rng.choice(rest, m - len(own), replace=False)]).astype(np.int64))
        idx.append(ids)
        val.append(rng.choice(VALUES, m))
        ptr.append(ptr[-1] + m)
    return VectorColumn(SIZE, torch.tensor(ptr, dtype=torch.int64),
                        torch.from_numpy(np.concatenate(idx).astype(np.int32)),
                        torch.from_numpy(np.concatenate(val)).to(dtype))


def hand_rows(ens: Ens, n: int = 40, seed: int = 1, dtype=torch.float64) -> VectorColumn:
    """Row 0 is empty; the others mix used and unused features; values often equal a threshold."""
    used = sorted({int(f) for t in ens.trees for f in t.feature if f >= 0})
    rng = np.random.default_rng(seed)
    return rows_with_nnz([0] + [int(rng.integers(1, 12)) for _ in range(n - 1)], used, seed, dtype)


# ------------------------------------------------------------------------------- the oracle
def oracle_tree(t: Tree, payload: str, k: int, cmp_less: bool, x: dict):
    """Brute-force Shapley values of one tree at ``x``: ({feature: phi}, v(empty set))."""
    st = t.stats.astype(np.float64)
    cover = st[:, 1] if payload == "value" else st.sum(1)

    def value(i):
        if payload == "value":
            return st[i, 0]
        return st[i, k] / cover[i] if payload == "normalized" else st[i, k]

    def v(i, S):
        f = int(t.feature[i])
        if f < 0:
            return value(i)
        lo, hi = int(t.left[i]), int(t.right[i])
        if f in S:
            xv = x.get(f, 0.0)
            return v(lo if (xv < t.threshold[i] if cmp_less else xv <= t.threshold[i]) else hi, S)
        return (cover[lo] * v(lo, S) + cover[hi] * v(hi, S)) / cover[i]

    feats = sorted({int(f) for f in t.feature if f >= 0})
    M = len(feats)
    assert M <= 8
    game = {frozenset(S): v(t.root, frozenset(S)) for r in range(M + 1) for S in itertools.combinations(feats, r)}
    phi = {}
    for f in feats:
        others = [g for g in feats if g != f]
        tot = 0.0
        for r in range(M):
            w = math.factorial(r) * math.factorial(M - r - 1) / math.factorial(M)
            for S in itertools.combinations(others, r):
                tot += w * (game[frozenset(S) | {f}] - game[frozenset(S)])
        phi[f] = tot
    return phi, game[frozenset()]


def oracle_ensemble(ens: Ens, k: int, vc: VectorColumn):
    """(phi [N, U] in the order of the sorted used features, bias)."""
    w = np.ones(len(ens.trees)) if ens.weights is None else ens.weights
    used = sorted({int(f) for t in ens.trees for f in t.feature if f >= 0})
    ptr, idx, val = (a.cpu().numpy() for a in vc.csr())
    phi = np.zeros((len(vc), len(used)))
    bias = 0.0
    for r in range(len(vc)):
        x = {int(f): float(v) for f, v in zip(idx[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]])}
        bias = 0.0          # v(empty set) does not depend on the row
        for wt, t in zip(w, ens.trees):
            p, b = oracle_tree(t, ens.payload, k, ens.cmp_less, x)
            bias += wt * b
            for f, c in p.items():
                phi[r, used.index(f)] += wt * c
    return phi, bias


def total_abs(paths) -> float:
    return float(np.abs(paths.path_v).sum())


def check_against_oracle(ens: Ens, k, vc, got: torch.Tensor):
    paths = ens.paths(k)
    want, bias = oracle_ensemble(ens, ens.K - 1 if k is None else k, vc)
    tol = REL_TOL * total_abs(paths)
    assert got.shape == want.shape
    assert np.abs(got.cpu().numpy() - want).max(initial=0.0) <= tol
    assert abs(paths.bias - bias) <= tol


# ------------------------------------------------------------------------------- CPU: the op
@pytest.mark.parametrize("name", sorted(HAND))
def test_oracle_agreement(name):
    ens = HAND[name]
    vc = hand_rows(ens)
    for k in ([None] if ens.K == 1 else [0, 1]):
        paths = ens.paths(k)
        got = tree_contributions(vc, paths)
        assert got.dtype == torch.float64 and got.shape == (len(vc), paths.features.size)
        check_against_oracle(ens, k, vc, got)
        # efficiency: contributions + bias = the scorer's output column
        score = score_csr(vc, ens.arrays())[:, ens.K - 1 if k is None else k]
        assert float((got.sum(1) + paths.bias - score).abs().max()) <= REL_TOL * total_abs(paths)


def test_values_equal_to_thresholds_follow_cmp_less():
    """x == threshold goes right under ``x < t`` and left under ``x <= t``."""
    t = stump(3, 1.0, -1.0, 2.0)
    vc = VectorColumn(SIZE, torch.tensor([0, 1]), torch.tensor([3], dtype=torch.int32), torch.tensor([1.0]).double())
    for cmp_less, leaf in ((True, 2.0), (False, -1.0)):
        ens = Ens([t], "value", None, cmp_less)
        got = tree_contributions(vc, ens.paths())
        check_against_oracle(ens, None, vc, got)
        assert float(got[0, 0]) + ens.paths().bias == pytest.approx(leaf, abs=1e-12)


def test_float32_values_and_unused_features():
    ens = HAND["random_value_lt"]
    vc64, vc32 = hand_rows(ens), hand_rows(ens, dtype=torch.float32)
    assert vc32.values.dtype == torch.float32
    a, b = tree_contributions(vc64, ens.paths()), tree_contributions(vc32, ens.paths())
    assert torch.equal(a, b)            # the pool's values are exact in float32
    # the empty row gets the all-missing attribution: every x_f counts as 0.0
    zero = VectorColumn(SIZE, torch.tensor([0, 1]), torch.tensor([SIZE - 1], dtype=torch.int32), torch.zeros(1).double())
    assert torch.equal(a[0], tree_contributions(zero, ens.paths())[0])


def test_thread_count_does_not_change_the_result():
    ens = HAND["normalized_weighted"]
    vc = hand_rows(ens, n=300, seed=5)
    one = tree_contributions(vc, ens.paths(), threads=1)
    assert torch.equal(one, tree_contributions(vc, ens.paths(), threads=16))
    assert torch.equal(one, tree_contributions(vc, ens.paths(), threads=3))


def test_path_table_layout():
    ens = HAND["one_feature_thrice_lt"]
    p = ens.paths()
    # four leaves, one element each (feature 5 merged), intervals [lo, hi) collapsed from the chain
    assert p.features.tolist() == [5] and p.path_ptr.tolist() == [0, 1, 2, 3, 4]
    assert p.pe_lo.tolist() == [-np.inf, 0.5, 1.0, 2.0] and p.pe_hi.tolist() == [0.5, 1.0, 2.0, np.inf]
    np.testing.assert_allclose(p.pe_z, [2 / 12, 3 / 12, 4 / 12, 3 / 12], rtol=1e-15)
    B = contrib_limits()["block_elems"]
    assert p.block_elems == B and p.slot_ptr.tolist() == [0, 4] and p.num_blocks == -(-4 // B)
    w = p.shapley.reshape(33, 32)
    assert w[1, 0] == 1.0 and w[3, 1] == pytest.approx(1 / 6) and w[32, 0] == 1 / 32
    assert all(abs(w[d, :d].sum() - sum(1 / math.comb(d - 1, k) for k in range(d)) / d) < 1e-15 for d in (2, 7, 32))


def test_limits():
    vc = rows_with_nnz([0, 5, 40], list(range(33)), seed=3)
    deep = Ens([chain(32)], "value", None, False)
    paths = deep.paths()
    assert int(np.diff(paths.path_ptr).max()) == 32
    got = tree_contributions(vc, paths)
    score = score_csr(vc, deep.arrays())[:, 0]
    assert float((got.sum(1) + paths.bias - score).abs().max()) <= REL_TOL * total_abs(paths)
    with pytest.raises(ValueError, match="32"):
        Ens([chain(33)], "value", None, False).paths()
    zero = stump(3, 1.0, -1.0, 2.0)
    zero.stats[0, 1] = 0.0
    with pytest.raises(ValueError, match="cover"):
        Ens([zero]).paths()
    with pytest.raises(ValueError):
        Ens([stump(3, 1.0, -1.0, 2.0)], "value").paths(output=1)
    with pytest.raises(ValueError):
        tree_contributions(VectorColumn(2, torch.tensor([0, 0])), Ens([stump(3, 1.0, -1.0, 2.0)]).paths())


def test_sanitized_host_twin_selftest():
    exe = _build.build_selftest("contrib", sanitize=True)
    res = subprocess.run([str(exe)], env={**os.environ, **_build.SELFTEST_ENV}, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "contrib selftest ok" in res.stdout


# ------------------------------------------------------------------------------- CPU: trained models
def _feature_stages():
    return [Tokenizer(inputCol="clean_text", outputCol="words"),
            StopWordsRemover(inputCol="words", outputCol="filtered_words"),
            HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
            IDF(inputCol="raw_features", outputCol="features")]


def _corpus(n, seed):
    pt, y = synth.generate(synth.SynthConfig(n=n, seed=seed))
    raw = TextColumn(pt.strings())
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})
    return Pipeline(stages=_feature_stages()).fit(df).transform(df)


@pytest.fixture(scope="module")
def trained():
    feats = _corpus(400, 11)
    return {"feats": feats,
            "xgb": SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=20,
                                      max_depth=6).fit(feats),
            "rf": RandomForestClassifier(featuresCol="features", labelCol="labels", numTrees=16, maxDepth=5,
                                         seed=42).fit(feats),
            "dt": DecisionTreeClassifier(featuresCol="features", labelCol="labels", maxDepth=5).fit(feats)}


def _host_column(frame) -> VectorColumn:
    vc = frame.column("features").to("cpu")
    return VectorColumn(vc.size, vc.indptr, vc.indices, vc.values)


@pytest.mark.parametrize("kind", ["xgb", "rf", "dt"])
def test_efficiency_on_trained_models(trained, kind):
    model, vc = trained[kind], _host_column(trained["feats"])
    paths = model.paths()
    tol = REL_TOL * total_abs(paths)
    phi = tree_contributions(vc, paths)
    score = score_csr(vc, model.scorer())
    assert float((phi.sum(1) + paths.bias - score[:, -1]).abs().max()) <= tol
    col = model.contributions(vc)
    assert isinstance(col, VectorColumn) and col.size == model.numFeatures + 1 and len(col) == len(vc)
    ptr, idx, val = col.csr()
    U = paths.features.size
    assert torch.equal(ptr, torch.arange(len(vc) + 1) * (U + 1))
    assert idx[:U + 1].tolist() == paths.features.tolist() + [model.numFeatures]
    raw1 = model.postprocess(score)[0][:, 1]           # rawPrediction[:, 1]
    if kind == "xgb":
        tol += REL_TOL * abs(model.base_margin)
    assert float((val.view(len(vc), U + 1).sum(1) - raw1).abs().max()) <= tol
    if kind == "dt":                                   # the class-1 count of the leaf reached
        x0 = dict(zip(vc.row(0).indices.tolist(), vc.row(0).values.tolist()))
        t = model.trees[0]
        assert float(val[:U + 1].sum()) == pytest.approx(t.stats[t.leaf_of(x0), 1], abs=tol)
    # a Frame works like its features column
    assert torch.equal(model.contributions(trained["feats"]).values.cpu(), val)


def test_booster_without_sum_hessian_has_no_contributions(trained):
    js = trained["xgb"].to_xgboost_json()
    back = SparkXGBClassifierModel.from_xgboost_json(js)
    vc = _host_column(trained["feats"])
    a = trained["xgb"].contributions(vc).values.view(len(vc), -1)
    b = back.contributions(vc).values.view(len(vc), -1)      # sum_hessian survives the JSON
    assert float((a - b).abs().max()) < 1e-5                  # (float32 thresholds and base score)
    for tj in js["learner"]["gradient_booster"]["model"]["trees"]:
        del tj["sum_hessian"]
    bare = SparkXGBClassifierModel.from_xgboost_json(js)
    with pytest.raises(ValueError, match="cover"):
        bare.contributions(vc)


def test_logistic_regression_contributions():
    rng = np.random.default_rng(2)
    w = rng.normal(size=SIZE)
    lr = LogisticRegressionModel(w, -0.375)
    vc = rows_with_nnz([0, 1, 7, 64], seed=4)
    col = lr.contributions(vc)
    assert col.size == SIZE + 1 and len(col) == 4
    ptr, idx, val = (a.numpy() for a in col.csr())
    sp, si, sv = (a.numpy() for a in vc.csr())
    margin = score_csr(vc, lr.scorer())[:, 0].numpy()
    for r in range(4):
        a, b = ptr[r], ptr[r + 1]
        assert idx[a:b].tolist() == si[sp[r]:sp[r + 1]].tolist() + [SIZE]
        np.testing.assert_array_equal(val[a:b - 1], w[si[sp[r]:sp[r + 1]]] * sv[sp[r]:sp[r + 1]])
        assert val[b - 1] == -0.375
        assert val[a:b].sum() == pytest.approx(margin[r], abs=1e-12 * (1 + np.abs(val[a:b]).sum()))
    multi = LogisticRegressionModel(w, 0.0, family="multinomial")
    with pytest.raises(NotImplementedError):
        multi.contributions(vc)


def test_pred_contrib_col(trained, tmp_path):
    model, feats = trained["xgb"], trained["feats"]
    assert not model.isSet("pred_contrib_col")
    plain = model.transform(feats)
    assert plain.columns == feats.columns + ["rawPrediction", "probability", "prediction"]
    # an unset model computes exactly what it did: attach_outputs of score_csr
    want = model.attach_outputs(feats, score_csr(feats.column("features"), model.scorer()))
    for c in ("rawPrediction", "probability", "prediction"):
        assert torch.equal(plain.column(c), want.column(c))
    with_col = model.copy()
    with_col.set("pred_contrib_col", "contribs")
    out = with_col.transform(feats)
    assert out.columns == plain.columns + ["contribs"]
    for c in ("rawPrediction", "probability", "prediction"):
        assert torch.equal(out.column(c), plain.column(c))
    col = out.column("contribs")
    assert torch.equal(col.values, model.contributions(feats).values)
    sums = col.values.view(len(col), -1).sum(1)
    tol = REL_TOL * (total_abs(model.paths()) + abs(model.base_margin))
    assert float((sums - out.column("rawPrediction")[:, 1]).abs().max()) <= tol
    with_col.save(str(tmp_path / "m"))
    back = SparkXGBClassifierModel.load(str(tmp_path / "m"))
    assert back.getOrDefault("pred_contrib_col") == "contribs"
    assert torch.equal(back.transform(feats).column("contribs").values, col.values)
    model.save(str(tmp_path / "plain"))
    md = json.loads((tmp_path / "plain" / "metadata" / "part-00000").read_text().splitlines()[0])
    assert "pred_contrib_col" not in md["paramMap"] and "pred_contrib_col" not in md.get("defaultParamMap", {})
    assert not SparkXGBClassifierModel.load(str(tmp_path / "plain")).isSet("pred_contrib_col")
    # the estimator hands the parameter to its model
    est = SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=2, max_depth=2,
                             pred_contrib_col="phi")
    assert "phi" in est.fit(feats).transform(feats).columns


# ------------------------------------------------------------------------------- CPU: agent
class RecordingLLM(StubLLM):
    def __init__(self):
        super().__init__()
        self.prompts = []

    def generate(self, prompt, temperature=0.7):
        self.prompts.append(prompt)
        return super().generate(prompt, temperature)


def _check_evidence(words, dialogue, stopwords, n):
    toks = set(text_oracle.remove_stopwords(text_oracle.tokenize(text_oracle.clean_text(dialogue)), stopwords))
    assert 0 < len(words) <= n
    for e in words:
        assert set(e) == {"word", "feature", "value", "contribution"}
        assert e["word"] and set(e["word"].split("/")) <= toks
    key = [(-abs(e["contribution"]), e["feature"]) for e in words]
    assert key == sorted(key)
    assert len({e["feature"] for e in words}) == len(words)


def test_agent_evidence_with_shipped_lr_pipeline(shipped_model_path, scam_sample):
    llm = RecordingLLM()
    agent = ClassificationAgent(str(shipped_model_path), llm=llm, device="cpu")
    words = agent.contributing_words(scam_sample, n=10)
    _check_evidence(words, scam_sample, agent.fused.stopwords, 10)
    lr = agent.fused.model
    for e in words:                                    # LR: contribution = w_f * x_f
        assert e["contribution"] == lr.coefficients[e["feature"]] * e["value"]
        assert text_oracle.term_index(e["word"].split("/")[0], agent.fused.dim) == e["feature"]
    assert [e["feature"] for e in agent.contributing_words(scam_sample, n=3)] == [e["feature"] for e in words[:3]]
    base = agent.classify_and_explain(scam_sample)
    assert set(base) == {"prediction", "confidence", "analysis", "historical_insight"}
    assert llm.prompts == [agent.analyzer.create_prompt(scam_sample, base["prediction"], base["confidence"])]
    zero = agent.classify_and_explain(scam_sample, evidence=0)
    assert zero == base and llm.prompts[1] == llm.prompts[0]
    ev = agent.classify_and_explain(scam_sample, evidence=5)
    assert set(ev) == set(base) | {"evidence"} and ev["evidence"] == words[:5]
    assert llm.prompts[2].startswith(llm.prompts[0]) and len(llm.prompts) == 3
    extra = llm.prompts[2][len(llm.prompts[0]):]
    assert extra.count("\n\n") == 1 and all(repr(e["word"]) in extra for e in words[:5])
    assert all(f"{e['contribution']:+.4g}" in extra for e in words[:5])


def test_agent_evidence_with_tree_pipeline(tmp_path, scam_sample):
    pt, y = synth.generate(synth.SynthConfig(n=400, seed=11))
    raw = TextColumn(pt.strings())
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})
    clf = SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=10, max_depth=4)
    Pipeline(stages=_feature_stages() + [clf]).fit(df).save(str(tmp_path / "m"))
    agent = ClassificationAgent(str(tmp_path / "m"), llm=StubLLM(), device="cpu")
    dialogue = pt.strings()[0]
    words = agent.contributing_words(dialogue, n=50)
    _check_evidence(words, dialogue, agent.fused.stopwords, 50)
    used = set(agent.fused.model.paths().features.tolist())
    assert {e["feature"] for e in words} <= used
    out = agent.classify_and_explain(dialogue, evidence=4, with_history=False)
    assert out["evidence"] == words[:4]


# ------------------------------------------------------------------------------- GPU
def both(vc, paths):
    """(host twin, device) results of the same call; the device result must equal it bitwise."""
    host = tree_contributions(vc, paths)
    dev = tree_contributions(vc.to("cuda:0"), paths)
    assert dev.is_cuda and dev.dtype == torch.float64
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), host)
    return host, dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_ensembles_match_host_and_oracle(name):
    ens = HAND[name]
    for dtype in (torch.float64, torch.float32):
        vc = hand_rows(ens, dtype=dtype)
        for k in ([None] if ens.K == 1 else [0, 1]):
            _, dev = both(vc, ens.paths(k))
            if dtype == torch.float64:
                check_against_oracle(ens, k, vc, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_gpu_path_count_at_the_chunk_edges(delta):
    chunk = contrib_limits()["paths_per_chunk"]
    for base in (chunk, 3 * chunk):
        want = base + delta
        rng = np.random.default_rng(want)
        trees = [stump(int(rng.integers(0, 50)), float(rng.choice(VALUES)), float(rng.normal()), float(rng.normal()))
                 for _ in range(want // 2)] + ([leaf_only(0.5)] if want % 2 else [])
        ens = Ens(trees)
        assert ens.paths().num_paths == want
        both(hand_rows(ens, n=70, seed=want), ens.paths())


@pytest.mark.gpu
def test_gpu_hot_feature_at_the_block_edges():
    B = contrib_limits()["block_elems"]
    rng = np.random.default_rng(0)
    for want in (B - 1, B, B + 1, 2 * B + 1):
        # stumps put two elements on the hot feature's slot, tri() three
        n_tri = want % 2
        trees = [tri(7, 9)] * n_tri + [stump(7, float(rng.choice(VALUES)), float(rng.normal()), float(rng.normal()))
                                       for _ in range((want - 3 * n_tri) // 2)]
        ens = Ens(trees)
        p = ens.paths()
        assert int(np.diff(p.slot_ptr)[p.features.tolist().index(7)]) == want
        host, _ = both(hand_rows(ens, n=70, seed=want), p)
        assert float((host.sum(1) + p.bias - score_csr(hand_rows(ens, n=70, seed=want), ens.arrays())[:, 0])
                     .abs().max()) <= REL_TOL * total_abs(p)


@pytest.mark.gpu
def test_gpu_row_lengths():
    ens = HAND["random_value_lt"]
    used = sorted({int(f) for t in ens.trees for f in t.feature if f >= 0})
    cap = contrib_limits()["lds_row_cap"]
    vc = rows_with_nnz([0, 1, 64, 65, 0, max(3000, min(cap + 1, SIZE)), 63, 129], used, seed=8)
    both(vc, ens.paths())


@pytest.mark.gpu
def test_gpu_row_counts_at_the_tile_and_group_edges():
    lim = contrib_limits()
    tile, group = lim["rows_per_tile"], lim["rows_per_group"]
    ens = HAND["leaf_and_trees"]
    vc = hand_rows(ens, n=tile + 1, seed=6)
    ptr, idx, val = vc.csr()
    for n in (1, 3, group - 1, group + 1, tile - 1, tile, tile + 1):    # 3 and tile - 1: no multiple of the 4 waves
        sub = VectorColumn(SIZE, ptr[:n + 1].clone(), idx[:int(ptr[n])].clone(), val[:int(ptr[n])].clone())
        host, _ = both(sub, ens.paths())
        assert host.shape[0] == n


@pytest.mark.gpu
def test_gpu_trained_gbdt_bitwise_and_repeatable():
    feats = _corpus(2048, 13)
    model = SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=20, max_depth=6).fit(feats)
    vc = _host_column(feats)
    paths = model.paths()
    host, dev = both(vc, paths)
    again = tree_contributions(vc.to("cuda:0"), paths)
    assert torch.equal(again, dev)
    score = score_csr(vc, model.scorer())[:, 0]
    assert float((host.sum(1) + paths.bias - score).abs().max()) <= REL_TOL * total_abs(paths)
    # the model API on the device column: same numbers, rows sum to rawPrediction[:, 1]
    col = model.contributions(vc.to("cuda:0"))
    assert torch.equal(col.values.view(len(vc), -1)[:, :-1], dev)
