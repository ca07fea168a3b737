"""``xgboost.spark.SparkXGBClassifier``-compatible estimator on the gfx950 GBDT engine (R-06, X-13).

Same constructor surface the reference uses (``features_col, label_col, num_workers, max_depth,
n_estimators, eval_metric``; /root/reference/fraud_detection_spark.py:76-83) plus the usual XGBoost
knobs. ``num_workers`` maps to data-parallel ranks: inside a ``torch.distributed`` job each rank
trains on its row shard and histograms are reduce-scattered over RCCL (the reference's Rabit
ring); from a single process ``num_workers > 1`` launches that many rank processes
(parallel/estimator_dp.py) and returns rank 0's model (identical on every rank).

Outputs follow xgboost.spark: ``rawPrediction = [-margin, margin]``, ``probability = [1-p, p]``,
``prediction = p > 0.5``. With ``objective="multi:softprob"`` (chosen by itself, as xgboost.spark does,
when the objective was not set, no process group is active and a label exceeds 1) the model holds
``C`` trees per round (models/gbdt_softprob.py): ``rawPrediction`` is the ``[N, C]`` margins,
``probability`` their max-subtracted softmax, ``prediction`` the first argmax. Models persist in the Spark ML layout (metadata + ``data/`` trees) and
export XGBoost JSON (``save_xgboost_json``; loadable by ``xgboost.Booster.load_model``).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from ..io import spark_format as sf
from ..ops.text import TreeArrays
from .base import Estimator, Param, register
from .classification import ClassificationModelBase
from .frame import Frame
from .tree_model import NODE_FIELDS, Tree, ensemble_arrays, ensemble_paths


MULTI_OBJECTIVE = "multi:softprob"


class _XGBParams:
    _params = [Param("features_col", "features column", "features", str),
               Param("label_col", "label column", "label", str),
               Param("prediction_col", "prediction column", "prediction", str),
               Param("probability_col", "probability column", "probability", str),
               Param("raw_prediction_col", "raw prediction column", "rawPrediction", str),
               Param("weight_col", "weight column", None, str, has_default=False),
               Param("pred_contrib_col", "feature-contribution (TreeSHAP) output column", None, str,
                     has_default=False),
               Param("validation_indicator_col", "boolean column: true rows form the validation set", None, str,
                     has_default=False),
               Param("early_stopping_rounds", "stop after this many rounds without a better validation metric",
                     None, int, has_default=False),
               Param("num_workers", "data-parallel workers", 1, int),
               Param("max_depth", "max tree depth", 6, int),
               Param("n_estimators", "boosting rounds", 100, int),
               Param("learning_rate", "eta", 0.3, float),
               Param("reg_lambda", "L2 regularisation", 1.0, float),
               Param("gamma", "min split loss", 0.0, float),
               Param("min_child_weight", "min hessian per child", 1.0, float),
               Param("max_bin", "histogram bins per feature", 256, int),
               Param("max_delta_step", "max leaf step", 0.0, float),
               Param("base_score", "initial prediction (None = estimated)", None, float, has_default=False),
               Param("eval_metric", "evaluation metric", "auc", str),
               Param("objective", "objective", "binary:logistic", str),
               Param("tree_method", "tree method", "hist", str),
               Param("seed", "random seed", 0, int),
               Param("subsample", "fraction of the rows each boosting round keeps, in (0, 1]", 1.0, float),
               Param("colsample_bytree", "fraction of the features each tree may split on, in (0, 1]", 1.0, float),
               Param("colsample_bylevel", "fraction of the tree's features each level may split on", 1.0, float),
               Param("colsample_bynode", "fraction of the level's features each node may split on", 1.0, float),
               Param("sampling_method", "row sampling method (only 'uniform')", "uniform", str),
               Param("deterministic", "accepted for compatibility: training is always bitwise reproducible", True,
                     bool)]

    # defaults that are not written to ``defaultParamMap``: the metadata of a model that never set
    # them keeps the bytes it had before these parameters existed (a set value goes to ``paramMap``)
    _persist_defaults_only = ("subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode",
                              "sampling_method")

    # ClassificationModelBase reads Spark-style column getters
    def getFeaturesCol(self):  # noqa: N802
        return self.getOrDefault("features_col")

    def getLabelCol(self):  # noqa: N802
        return self.getOrDefault("label_col")

    def getPredictionCol(self):  # noqa: N802
        return self.getOrDefault("prediction_col")

    def getProbabilityCol(self):  # noqa: N802
        return self.getOrDefault("probability_col")

    def getRawPredictionCol(self):  # noqa: N802
        return self.getOrDefault("raw_prediction_col")


def _as_numpy(col):
    if isinstance(col, torch.Tensor):
        return col.cpu().numpy()
    return np.asarray(list(col) if not isinstance(col, np.ndarray) else col)


def split_validation(X, y, w, mask):
    """(validation features, labels, weights, training features, labels, weights): rows with a
    true ``mask`` validate, the rest train; the weight column is split the same way."""
    mask = np.asarray(mask).astype(bool)
    vi, ti = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    yy = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray([float(v) for v in y], dtype=np.float32))
    ww = None if w is None else np.asarray(_as_numpy(w), dtype=np.float32)

    def part(ix):
        return X.take(ix), yy[torch.from_numpy(ix).to(yy.device)], None if ww is None else ww[ix]

    return (*part(vi), *part(ti))


@register("xgboost.spark.core.SparkXGBClassifier")
class SparkXGBClassifier(_XGBParams, Estimator):
    _uid_prefix = "SparkXGBClassifier"

    def __init__(self, **kw):
        kw = {("learning_rate" if k == "eta" else k): v for k, v in kw.items()}
        super().__init__(**kw)

    def _fit(self, frame: Frame) -> "SparkXGBClassifierModel":
        from ..models.gbdt import GBDTParams, check_sampling, fit_gbdt

        objective = self.getOrDefault("objective")
        if objective not in ("binary:logistic", MULTI_OBJECTIVE):
            raise NotImplementedError("only objective='binary:logistic' and 'multi:softprob' are supported")
        if self.getOrDefault("sampling_method") != "uniform":
            raise NotImplementedError("only sampling_method='uniform' is supported")
        p = GBDTParams(n_estimators=self.getOrDefault("n_estimators"), max_depth=self.getOrDefault("max_depth"),
                       learning_rate=self.getOrDefault("learning_rate"), reg_lambda=self.getOrDefault("reg_lambda"),
                       gamma=self.getOrDefault("gamma"), min_child_weight=self.getOrDefault("min_child_weight"),
                       max_bin=self.getOrDefault("max_bin"), max_delta_step=self.getOrDefault("max_delta_step"),
                       base_score=self._paramMap.get("base_score"), seed=self.getOrDefault("seed"),
                       deterministic=bool(self.getOrDefault("deterministic")),
                       subsample=self.getOrDefault("subsample"),
                       colsample_bytree=self.getOrDefault("colsample_bytree"),
                       colsample_bylevel=self.getOrDefault("colsample_bylevel"),
                       colsample_bynode=self.getOrDefault("colsample_bynode"))
        check_sampling(p)
        w = frame.column(self.getOrDefault("weight_col")) if self.isSet("weight_col") else None
        X, y = frame.column(self.getFeaturesCol()), frame.column(self.getLabelCol())
        if objective == MULTI_OBJECTIVE or self._labels_exceed_one(y):
            return self._fit_softprob(X, y, w, p)
        # validation rows (xgboost.spark's validation_indicator_col): split off before training, so
        # the base score, bins and trees are those of a fit on the remaining rows alone.
        # eval_metric is read only here
        mask, ev = None, {}
        if self.isSet("validation_indicator_col"):
            from ..models.monitor import check_eval_args

            mask = np.asarray(_as_numpy(frame.column(self.getOrDefault("validation_indicator_col")))).astype(bool)
            ev = dict(eval_metric=self.getOrDefault("eval_metric"),
                      early_stopping_rounds=self._paramMap.get("early_stopping_rounds"))
            check_eval_args((None, None, w if mask.any() else None), ev["eval_metric"], ev["early_stopping_rounds"])
            if not mask.any():
                raise ValueError("the validation set is empty")
        from ..parallel import dist as D
        from ..parallel.estimator_dp import effective_workers

        from ..utils.config import default_device

        dev = default_device()
        nw = effective_workers(self.getOrDefault("num_workers"), len(X), dev, nnz=X.nnz)
        if nw > 1 and not D.is_dist():
            # N rank processes (one per GPU over RCCL, else gloo CPU ranks) behind the watchdog
            from dataclasses import asdict

            from ..parallel.estimator_dp import fit_data_parallel

            out, self.last_dp_report = fit_data_parallel("gbdt", X, y, w, asdict(p), nw, device=dev,
                                                         valid_mask=mask, eval_kw=ev)
            (trees, nf, base, secs), hist = out[:4], (out[4] if len(out) > 4 else {})
        else:          # one process, or already one rank of a torchrun job
            if mask is not None:
                Xv, yv, wv, X, y, w = split_validation(X, y, w, mask)
                res = fit_gbdt(X, y, p, weights=w, device=dev, eval_set=(Xv, yv, wv), **ev)
            else:
                res = fit_gbdt(X, y, p, weights=w, device=dev)
            trees, nf, base, secs = res.trees, res.num_features, res.base_margin, res.train_seconds
            hist = dict(evals_result=res.evals_result, best_iteration=res.best_iteration, best_score=res.best_score)
        m = SparkXGBClassifierModel(trees, nf, base, uid=self.uid)
        if mask is not None:
            m.evals_result, m.best_iteration, m.best_score = hist["evals_result"], hist["best_iteration"], \
                hist["best_score"]
        m._paramMap.update(self._paramMap)
        m.training_seconds = secs
        return m


    def _labels_exceed_one(self, y) -> bool:
        """Whether the default route must hand over to ``multi:softprob``: this process's labels hold a
        value above 1 (read on the host: no launch, no collective). An explicit ``binary:logistic``
        with such a label is an error; under an ambient process group the objective is never chosen
        here (the ranks see different labels), it has to be set."""
        from ..parallel import dist as D

        yy = np.asarray(_as_numpy(y), dtype=np.float64).reshape(-1)
        above = bool(yy.size) and bool(np.nanmax(yy) > 1.0)
        if not above:
            return False
        if self.isSet("objective"):
            raise ValueError("objective='binary:logistic' needs labels in {0, 1}; the label column holds "
                             f"{np.nanmax(yy):g} (leave the objective unset or use 'multi:softprob')")
        if D.is_dist():
            raise ValueError("the label column holds a value above 1: under a process group the objective is not "
                             "chosen from the local labels, set objective='multi:softprob'")
        return True

    def _fit_softprob(self, X, y, w, p) -> "SparkXGBClassifierModel":
        """The multi-class route (models/gbdt_softprob.py); one process, or one rank of an ambient
        process group."""
        from ..models.gbdt_softprob import fit_gbdt_softprob
        from ..utils.config import default_device

        for name in ("validation_indicator_col", "early_stopping_rounds", "pred_contrib_col"):
            if self.isSet(name):
                raise NotImplementedError(f"{name} is not supported with objective='multi:softprob'")
        if int(self.getOrDefault("num_workers")) > 1:
            raise NotImplementedError("num_workers > 1 is not supported with objective='multi:softprob' (data "
                                      "parallelism there runs through the ambient process group)")
        res = fit_gbdt_softprob(X, y, p, weights=w, device=default_device())
        m = SparkXGBClassifierModel(res.trees, res.num_features, res.base_margin, num_class=res.num_class, uid=self.uid)
        m._paramMap.update(self._paramMap)
        m._paramMap["objective"] = MULTI_OBJECTIVE
        m.training_seconds = res.train_seconds
        return m


@register("xgboost.spark.core.SparkXGBClassifierModel")
class SparkXGBClassifierModel(_XGBParams, ClassificationModelBase):
    _uid_prefix = "SparkXGBClassifierModel"

    def __init__(self, trees=None, num_features: int = 0, base_margin: float = 0.0, num_class: int = 0,
                 tree_class=None, **kw):
        """``num_class``: 0 for a ``binary:logistic`` booster (xgboost's own convention), else the
        class count of a ``multi:softprob`` booster whose tree ``i`` belongs to class ``tree_class[i]``
        (default ``i % num_class``, the training order)."""
        super().__init__(**kw)
        self._set_classes(num_class, tree_class, len(trees or []))
        self._trees = list(trees or [])
        self._num_features = int(num_features)
        self.base_margin = float(base_margin)
        self._arrays: Optional[TreeArrays] = None
        self.training_seconds = 0.0
        # validation monitoring (fit with validation_indicator_col), as xgboost names them
        self.best_iteration: Optional[int] = None
        self.best_score: Optional[float] = None
        self.evals_result: dict = {}

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return self._num_features

    @property
    def trees(self) -> list:
        return self._trees

    def _set_classes(self, num_class: int, tree_class, n_trees: int) -> None:
        from ..ops.sparse import softprob_limits

        self.num_class = int(num_class)
        self.numClasses = self.num_class if self.num_class > 0 else 2
        self._tree_class = None
        self._class_arrays = None
        if self.num_class == 0:
            return
        lim = int(softprob_limits()["max_classes"])
        if not 2 <= self.num_class <= lim:
            raise ValueError(f"num_class must be 0 (binary) or lie in 2 .. {lim}, got {num_class}")
        tc = np.arange(n_trees) % self.num_class if tree_class is None else np.asarray(tree_class, dtype=np.int64)
        if tc.size != n_trees or (tc.size and (tc.min() < 0 or tc.max() >= self.num_class)):
            raise ValueError("tree_class needs one class id in 0 .. num_class - 1 per tree")
        self._tree_class = tc.astype(np.int32)

    @property
    def isMulticlass(self) -> bool:  # noqa: N802
        """A ``multi:softprob`` booster (also one of two classes: its outputs are ``[N, 2]`` margins)."""
        return getattr(self, "num_class", 0) > 0

    def class_tree_scorer(self):
        """The class-grouped tree list of a ``multi:softprob`` model (``ops.sparse.score_class_trees``)."""
        from .tree_model import class_ensemble_arrays

        if not self.isMulticlass:
            raise ValueError("class_tree_scorer() belongs to a multi:softprob model; a binary model has scorer()")
        if self._class_arrays is None:
            self._class_arrays = class_ensemble_arrays(self._trees, self._tree_class, self.num_class, cmp_less=True)
        return self._class_arrays

    def _no_margin(self, what: str):
        return ValueError(f"{what} describes the single margin of a binary model; this multi:softprob model has "
                          f"{self.numClasses} classes (use transform / class_tree_scorer())")

    def serving_scorer(self):
        if self.isMulticlass:
            raise NotImplementedError("the fused class-tree tail is missing: multi:softprob tree models are served "
                                      "by transform() only (README, Multi-class boosting)")
        return self.scorer()

    def scorer(self) -> TreeArrays:
        if self.isMulticlass:
            raise self._no_margin("scorer()")
        if self._arrays is None:
            # thresholds are midpoints between bin values: "<" and "<=" agree on all seen values;
            # keep XGBoost's "x < split_condition" semantics
            self._arrays = ensemble_arrays(self._trees, "value", None, cmp_less=True)
        return self._arrays

    def paths(self):
        """TreeSHAP path table of the margin, cached with (and as long as) the scorer's arrays."""
        if self.isMulticlass:
            raise self._no_margin("paths()")
        arrays = self.scorer()
        cached = self.__dict__.get("_paths")
        if cached is None or cached[0] is not arrays:
            cached = self._paths = (arrays, ensemble_paths(self._trees, "value", None, cmp_less=True))
        return cached[1]

    def contributions(self, features):
        """Feature contributions to the margin; the bias entry includes ``base_margin``, so a row
        sums to ``rawPrediction[:, 1]`` (xgboost's ``pred_contribs``)."""
        if self.isMulticlass:
            raise NotImplementedError("TreeSHAP contributions of multi:softprob models are not supported")
        paths = self.paths()
        return self._tree_contributions(features, paths, paths.bias + self.base_margin)

    def _class_raw(self, vc) -> torch.Tensor:
        from ..ops.sparse import score_class_trees

        return score_class_trees(vc, self.class_tree_scorer())

    def _transform(self, frame: Frame) -> Frame:
        if self.isMulticlass:
            if self.isSet("pred_contrib_col"):
                raise NotImplementedError("pred_contrib_col is not supported with objective='multi:softprob'")
            return self.attach_outputs(frame, self._class_raw(self._features_column(frame)))
        out = super()._transform(frame)
        if self.isSet("pred_contrib_col"):
            out = out.withColumn(self.getOrDefault("pred_contrib_col"), self.contributions(frame))
        return out

    def predict(self, features) -> float:
        if not self.isMulticlass:
            return super().predict(features)
        from .linalg import VectorColumn

        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return float(self.postprocess(self._class_raw(vc))[2][0])

    def predictProbability(self, features):  # noqa: N802
        if not self.isMulticlass:
            return super().predictProbability(features)
        from .linalg import DenseVector, VectorColumn

        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self.postprocess(self._class_raw(vc))[1][0].cpu().numpy())

    def postprocess(self, raw: torch.Tensor):
        if self.isMulticlass:
            if raw.dim() != 2 or raw.shape[1] != self.numClasses:
                raise ValueError(f"expected [N, {self.numClasses}] class scores")
            m = raw + self.base_margin
            e = torch.exp(m - m.max(dim=1, keepdim=True).values)
            prob = e / e.sum(dim=1, keepdim=True)
            return m, prob, torch.argmax(prob, dim=1).to(torch.float64)   # (the first argmax on ties)
        m = raw[:, 0] + self.base_margin
        rp = torch.stack([-m, m], dim=1)
        p = torch.sigmoid(m)
        prob = torch.stack([1.0 - p, p], dim=1)
        return rp, prob, (p > 0.5).to(torch.float64)

    def postprocess_numpy(self, raw: np.ndarray):
        if self.isMulticlass:
            return ClassificationModelBase.postprocess_numpy(self, raw)
        m = raw[:, 0] + self.base_margin
        p = np.exp(-m)
        np.add(p, 1.0, out=p)
        np.reciprocal(p, out=p)
        return (m > 0.0).astype(np.float64), p

    def get_booster(self):
        return self

    @property
    def featureImportances(self):  # noqa: N802
        """XGBoost ``total_gain`` importance, normalised (used by word-association analysis)."""
        from .linalg import SparseVector

        imp = np.zeros(self._num_features)
        for t in self._trees:
            for i in range(t.num_nodes):
                if t.feature[i] >= 0:
                    imp[t.feature[i]] += t.gain[i]
        s = imp.sum()
        if s > 0:
            imp /= s
        nz = np.nonzero(imp)[0]
        return SparseVector(self._num_features, nz, imp[nz])

    # ------------------------------------------------------------ persistence
    def _metadata_extra(self):
        md = {"numFeatures": self._num_features, "numClasses": self.numClasses, "numTrees": len(self._trees),
              "baseMargin": self.base_margin}
        if getattr(self, "best_iteration", None) is not None:
            md.update(bestIteration=int(self.best_iteration), bestScore=float(self.best_score),
                      evalsResult=self.evals_result)
        return md

    def _save_data(self, path) -> None:
        """xgboost.spark's writer layout: ``metadata/`` (Spark DefaultParamsWriter JSON, written by
        the base class) and ``model/part-00000`` — the booster JSON as a one-line text part, what
        ``SparkXGBModelWriter`` writes with ``saveAsTextFile``. The fp64 split thresholds and node
        statistics of this engine ride in ``learner.attributes["fdx_trees"]`` (XGBoost keeps
        string attributes and ignores unknown ones) so a reload scores bitwise identically."""
        d = Path(path) / "model"
        d.mkdir(parents=True, exist_ok=True)
        booster = self.to_xgboost_json()
        booster["learner"]["attributes"]["fdx_trees"] = json.dumps([t.to_node_rows() for t in self._trees])
        booster["learner"]["attributes"]["fdx_base_margin"] = repr(self.base_margin)
        if self.isMulticlass:
            booster["learner"]["attributes"]["fdx_num_class"] = str(self.num_class)
        (d / "part-00000").write_text(json.dumps(booster) + "\n")
        (d / "_SUCCESS").write_text("")

    def _load_data(self, path, md) -> None:
        """Reads the xgboost.spark layout (``model/`` text part), and the earlier layout of this
        package (``data/`` parquet node rows)."""
        part = Path(path) / "model" / "part-00000"
        if part.exists():
            booster = json.loads(part.read_text().splitlines()[0])
            attrs = booster["learner"].get("attributes", {})
            if "fdx_trees" in attrs:
                self._trees = [Tree.from_node_rows(rows) for rows in json.loads(attrs["fdx_trees"])]
                self.base_margin = float(attrs["fdx_base_margin"])
                self._num_features = int(booster["learner"]["learner_model_param"]["num_feature"])
                nc = int(attrs.get("fdx_num_class", 0))
                self._set_classes(nc, booster["learner"]["gradient_booster"]["model"]["tree_info"] if nc else None,
                                  len(self._trees))
            else:                                   # a booster written by xgboost itself
                other = SparkXGBClassifierModel.from_xgboost_json(booster)
                self._trees, self._num_features, self.base_margin = other._trees, other._num_features, \
                    other.base_margin
                self._set_classes(other.num_class, other._tree_class, len(self._trees))
        else:
            rows = sf.read_data_parquet(path).to_pylist()
            by_tree: dict = {}
            for r in rows:
                by_tree.setdefault(r["treeID"], []).append(r["nodeData"])
            self._trees = [Tree.from_node_rows(by_tree[k]) for k in sorted(by_tree)]
            self._num_features = int(md.get("numFeatures", 0))
            self.base_margin = float(md.get("baseMargin", 0.0))
            self._set_classes(0, None, len(self._trees))
        self._arrays = None
        self.training_seconds = 0.0
        self.best_iteration = int(md["bestIteration"]) if "bestIteration" in md else None
        self.best_score = float(md["bestScore"]) if "bestScore" in md else None
        self.evals_result = md.get("evalsResult", {})

    def _save_data_legacy(self, path) -> None:
        """The round-1 layout (``data/`` parquet node rows + ``xgboost_model.json``), kept for tests
        of the backward-compatible reader."""
        rows = [{"treeID": t, "nodeData": r} for t, tree in enumerate(self._trees) for r in tree.to_node_rows()]
        sf.write_data_parquet(path, [sf.Field.simple("treeID", "integer"), sf.Field.struct("nodeData", NODE_FIELDS)],
                              rows)
        self.save_xgboost_json(Path(path) / "xgboost_model.json")

    def to_xgboost_json(self) -> dict:
        """XGBoost >= 1.6 JSON model (gbtree, binary:logistic). Split conditions are float32 in
        XGBoost; ours are fp64 midpoints, rounded here (exact for integer-count features)."""
        trees = []
        for tid, t in enumerate(self._trees):
            t = t.compacted()
            n = t.num_nodes
            leaf = t.feature < 0
            parents = np.full(n, 2147483647, dtype=np.int64)
            for i in range(n):
                if not leaf[i]:
                    parents[t.left[i]] = i
                    parents[t.right[i]] = i
            trees.append({
                "base_weights": [float(v) for v in np.where(leaf, t.stats[:, 0], 0.0)],
                "categories": [], "categories_nodes": [], "categories_segments": [], "categories_sizes": [],
                # rows absent from a sparse input carry value 0: route them like a stored 0
                "default_left": [int(leaf[i] or 0.0 < float(np.float32(t.threshold[i]))) for i in range(n)],
                "id": tid,
                "left_children": [int(v) for v in np.where(leaf, -1, t.left)],
                "right_children": [int(v) for v in np.where(leaf, -1, t.right)],
                "loss_changes": [float(v) if not leaf[i] else 0.0 for i, v in enumerate(t.gain)],
                "parents": [int(v) for v in parents],
                "split_conditions": [float(np.float32(t.threshold[i])) if not leaf[i] else float(t.stats[i, 0])
                                     for i in range(n)],
                "split_indices": [int(v) if v >= 0 else 0 for v in t.feature],
                "split_type": [0] * n,
                "sum_hessian": [float(v) for v in t.stats[:, 1]],
                "tree_param": {"num_deleted": "0", "num_feature": str(self._num_features), "num_nodes": str(n),
                               "size_leaf_vector": "1"},
            })
        attrs = {}
        if getattr(self, "best_iteration", None) is not None:       # (strings, as xgboost writes them)
            attrs = {"best_iteration": str(int(self.best_iteration)), "best_score": repr(float(self.best_score))}
        if self.isMulticlass:
            # multi:softprob: the base score is the margin itself (no logit), tree_info names each tree's
            # class and an iteration holds num_class trees: iteration_indptr = [0, C, 2C, ...]
            nc, tc = str(self.num_class), [int(c) for c in self._tree_class]
            indptr = sorted(set(range(0, len(tc), self.num_class)) | {len(tc)})
            return {
                "learner": {
                    "attributes": attrs,
                    "feature_names": [], "feature_types": [],
                    "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1",
                                                                          "num_trees": str(len(trees))},
                                                   "iteration_indptr": indptr,
                                                   "tree_info": tc, "trees": trees},
                                         "name": "gbtree"},
                    "learner_model_param": {"base_score": f"{self.base_margin:.9E}", "boost_from_average": "1",
                                            "num_class": nc, "num_feature": str(self._num_features),
                                            "num_target": "1"},
                    "objective": {"name": MULTI_OBJECTIVE, "softmax_multiclass_param": {"num_class": nc}},
                },
                "version": [2, 0, 3],
            }
        base_p = 1.0 / (1.0 + np.exp(-self.base_margin))
        return {
            "learner": {
                "attributes": attrs,
                "feature_names": [], "feature_types": [],
                "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1",
                                                                      "num_trees": str(len(trees))},
                                               "iteration_indptr": list(range(len(trees) + 1)),
                                               "tree_info": [0] * len(trees), "trees": trees},
                                     "name": "gbtree"},
                "learner_model_param": {"base_score": f"{base_p:.9E}", "boost_from_average": "1",
                                        "num_class": "0", "num_feature": str(self._num_features),
                                        "num_target": "1"},
                "objective": {"name": "binary:logistic", "reg_loss_param": {"scale_pos_weight": "1"}},
            },
            "version": [2, 0, 3],
        }

    def save_xgboost_json(self, path) -> None:
        Path(path).write_text(json.dumps(self.to_xgboost_json()))

    @classmethod
    def from_xgboost_json(cls, path_or_dict) -> "SparkXGBClassifierModel":
        d = path_or_dict if isinstance(path_or_dict, dict) else json.loads(Path(path_or_dict).read_text())
        L = d["learner"]
        nf = int(L["learner_model_param"]["num_feature"])
        bp = float(L["learner_model_param"]["base_score"])
        nc = int(L["learner_model_param"].get("num_class", 0) or 0)
        # (multi:softprob: the base score is the margin, untransformed)
        base = bp if nc > 0 else float(np.log(bp / (1 - bp)))
        trees = []
        for tj in L["gradient_booster"]["model"]["trees"]:
            lc = np.asarray(tj["left_children"])
            rc = np.asarray(tj["right_children"])
            leaf = lc < 0
            n = lc.size
            cond = np.asarray(tj["split_conditions"], dtype=np.float64)
            feat = np.where(leaf, -1, np.asarray(tj["split_indices"])).astype(np.int32)
            val = np.where(leaf, cond, 0.0)
            hess = np.asarray(tj.get("sum_hessian", [0.0] * n), dtype=np.float64)
            trees.append(Tree(feat, np.where(leaf, 0.0, cond), np.where(leaf, -1, lc).astype(np.int32),
                              np.where(leaf, -1, rc).astype(np.int32), np.stack([val, hess], 1), np.zeros(n),
                              np.asarray(tj["loss_changes"], dtype=np.float64), np.zeros(n, np.int64), val, 0))
        if nc > 0:
            return cls(trees, nf, base, num_class=nc, tree_class=L["gradient_booster"]["model"]["tree_info"])
        return cls(trees, nf, base)
