"""Classifiers: LogisticRegression, LinearSVC, DecisionTreeClassifier, RandomForestClassifier, NaiveBayes (+ models).

Models score through the native engine: either fused with the text featurizer
(``ml.fused``; one gfx950 launch from raw bytes to scores) or over an existing feature column
(``ops.sparse.score_csr``). Output columns follow Spark's ProbabilisticClassificationModel:
``rawPrediction`` [N,2], ``probability`` [N,2], ``prediction`` [N] (float64).

Reference: classifiers built at /root/reference/fraud_detection_spark.py:59-83; the shipped
LogisticRegressionModel stage (dialogue_classification_model/stages/4_LogisticRegression_*).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..io import spark_format as sf
from ..ops.text import ClassLinearScorer, LinearScorer, TreeArrays
from .base import Estimator, Model, Param, register
from .frame import Frame
from .linalg import DenseVector, VectorColumn
from .tree_model import NODE_FIELDS, Tree, ensemble_arrays, ensemble_paths, feature_importances


class _PredictorParams:
    _params = [Param("featuresCol", "features column name", "features", str),
               Param("labelCol", "label column name", "label", str),
               Param("predictionCol", "prediction column name", "prediction", str),
               Param("rawPredictionCol", "raw prediction column name", "rawPrediction", str),
               Param("probabilityCol", "probability column name", "probability", str)]


class ClassificationModelBase(_PredictorParams, Model):
    """Common scoring glue. Subclasses provide ``scorer()`` and ``postprocess(raw)``."""

    numClasses = 2

    def scorer(self):
        raise NotImplementedError

    @property
    def numFeatures(self) -> int:  # noqa: N802
        raise NotImplementedError

    def postprocess(self, raw: torch.Tensor):
        """raw kernel output [N, K] fp64 -> (rawPrediction [N,2], probability [N,2], prediction [N])."""
        raise NotImplementedError

    def postprocess_numpy(self, raw: np.ndarray):
        """Streaming hot path: raw [N, K] fp64 numpy -> (prediction [N], P(class 1) [N])."""
        _, prob, pred = self.postprocess(torch.from_numpy(raw))
        return pred.numpy(), prob[:, 1].numpy()

    def serving_scorer(self):
        """The scorer of the serving paths (``FusedPipeline(multiclass=True)``, the agent, the
        streaming engine): ``scorer()``, or the ``ClassLinearScorer`` of a model with more than two
        classes (``scorer()`` itself keeps raising for those)."""
        return self.scorer()

    def serving_postprocess(self, raw: np.ndarray):
        """Streaming hot path of ``serving_scorer()``'s output: raw [N, K] fp64 numpy -> (prediction [N],
        confidence [N]). For the ``[N, numClasses]`` class scores of a model with more than two classes
        ``prediction`` is ``postprocess``'s decision (the first argmax of the probability, or of
        ``p_c / t_c`` under NaiveBayes ``thresholds``) and ``confidence`` the probability of the predicted
        class; in every other case this is ``postprocess_numpy``: ``confidence = P(class 1)``."""
        if self.numClasses > 2 and raw.ndim == 2 and raw.shape[1] == self.numClasses:
            _, prob, pred = self.postprocess(torch.from_numpy(np.ascontiguousarray(raw)))
            pred, prob = pred.numpy(), prob.numpy()
            return pred, prob[np.arange(prob.shape[0]), pred.astype(np.int64)]
        return self.postprocess_numpy(raw)

    def _transform(self, frame: Frame) -> Frame:
        from ..ops.sparse import score_csr

        vc = frame.column(self.getFeaturesCol())
        if not isinstance(vc, VectorColumn):
            vc = VectorColumn.from_rows(list(vc))
        if vc.size < self.numFeatures:
            raise ValueError(f"features have size {vc.size}, model expects {self.numFeatures}")
        raw = score_csr(vc, self.scorer())
        return self.attach_outputs(frame, raw)

    def attach_outputs(self, frame: Frame, raw: torch.Tensor) -> Frame:
        rp, prob, pred = self.postprocess(raw)
        if self.getRawPredictionCol():
            frame = frame.withColumn(self.getRawPredictionCol(), rp)
        if self.getProbabilityCol():
            frame = frame.withColumn(self.getProbabilityCol(), prob)
        return frame.withColumn(self.getPredictionCol(), pred)

    def _features_column(self, features) -> VectorColumn:
        vc = features.column(self.getFeaturesCol()) if isinstance(features, Frame) else features
        if not isinstance(vc, VectorColumn):
            vc = VectorColumn.from_rows(list(vc))
        if vc.size < self.numFeatures:
            raise ValueError(f"features have size {vc.size}, model expects {self.numFeatures}")
        return vc

    def contributions(self, features) -> VectorColumn:
        """Per-row feature contributions to the class-1 raw score of ``features`` (a ``VectorColumn``
        or a ``Frame`` holding ``featuresCol``): a CSR column of size ``numFeatures + 1`` whose last
        index ``numFeatures`` is the bias; a row sums to the score. Binary models only."""
        raise NotImplementedError

    def _tree_contributions(self, features, paths, bias: float) -> VectorColumn:
        """Tree models: every row stores the ensemble's used features (ascending), then the bias."""
        from ..ops.sparse import tree_contributions

        vc = self._features_column(features)
        phi = tree_contributions(vc, paths)
        n, nf, dev = phi.shape[0], self.numFeatures, phi.device
        val = torch.cat([phi, torch.full((n, 1), bias, dtype=torch.float64, device=dev)], dim=1)
        idx = torch.cat([torch.from_numpy(paths.features), torch.tensor([nf], dtype=torch.int32)]).to(dev)
        indptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * val.shape[1]
        return VectorColumn(nf + 1, indptr, idx.repeat(n), val.reshape(-1))

    def predict(self, features) -> float:
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        from ..ops.sparse import score_csr

        return float(self.postprocess(score_csr(vc, self.scorer()))[2][0])

    def predictProbability(self, features) -> DenseVector:  # noqa: N802
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        from ..ops.sparse import score_csr

        return DenseVector(self.postprocess(score_csr(vc, self.scorer()))[1][0].cpu().numpy())


def _argmax_prediction(prob: torch.Tensor) -> torch.Tensor:
    return torch.argmax(prob, dim=1).to(torch.float64)   # first max index on ties (Vector.argmax)


def _normalize(raw: torch.Tensor) -> torch.Tensor:
    s = raw.sum(1, keepdim=True)
    return torch.where(s != 0, raw / torch.where(s != 0, s, torch.ones_like(s)), raw)


def _linear_contributions(vc: VectorColumn, weights: torch.Tensor, bias: float, nf: int) -> VectorColumn:
    """Linear models: every row stores its own entries ``w_f * x_f``, then ``bias`` at index ``nf``."""
    indptr, idx, val = vc.csr()
    dev, n = indptr.device, indptr.numel() - 1
    rows = torch.arange(n + 1, dtype=torch.int64, device=dev)
    row_of = torch.repeat_interleave(rows[:-1], indptr[1:] - indptr[:-1], output_size=int(idx.numel()))
    out_idx = torch.full((int(idx.numel()) + n,), nf, dtype=torch.int32, device=dev)
    out_val = torch.full((int(idx.numel()) + n,), bias, dtype=torch.float64, device=dev)
    pos = torch.arange(int(idx.numel()), dtype=torch.int64, device=dev) + row_of
    out_idx[pos] = idx.to(torch.int32)
    out_val[pos] = weights[idx.to(torch.int64)] * val.to(torch.float64)
    return VectorColumn(nf + 1, indptr + rows, out_idx, out_val)


# ============================================================================ logistic regression
class _LRParams(_PredictorParams):
    _params = [Param("family", "binomial|multinomial|auto", "auto", str),
               Param("fitIntercept", "fit an intercept", True, bool),
               Param("tol", "convergence tolerance", 1e-6, float),
               Param("standardization", "standardize features", True, bool),
               Param("maxIter", "max iterations", 100, int),
               Param("maxBlockSizeInMB", "block size", 0.0, float),
               Param("aggregationDepth", "treeAggregate depth", 2, int),
               Param("elasticNetParam", "L1 ratio", 0.0, float),
               Param("threshold", "binary threshold", 0.5, float),
               Param("regParam", "regularization", 0.0, float),
               Param("weightCol", "weight column", None, str, has_default=False)]

    _DEFAULT_ORDER = ("family", "predictionCol", "fitIntercept", "tol", "featuresCol", "standardization",
                      "maxIter", "maxBlockSizeInMB", "rawPredictionCol", "labelCol", "probabilityCol",
                      "aggregationDepth", "elasticNetParam", "threshold", "regParam")

    def _default_hook(self) -> None:
        d = self._defaultParamMap
        self._defaultParamMap = {k: d[k] for k in self._DEFAULT_ORDER if k in d}


@register("org.apache.spark.ml.classification.LogisticRegression")
class LogisticRegression(_LRParams, Estimator):
    """Spark's ``LogisticRegression``. ``family="binomial"`` (or ``"auto"`` on labels in {0, 1}) fits
    one coefficient row by L-BFGS / OWL-QN; ``family="multinomial"`` (or ``"auto"`` on labels
    ``0 .. C - 1`` with ``C > 2``) fits ``C <= 8`` rows with an L2 penalty on the fused fixed-point
    pass of ``models/lr.py::train_multinomial_logistic_regression``."""
    _uid_prefix = "LogisticRegression"

    def _fit(self, frame: Frame) -> "LogisticRegressionModel":
        from ..models.lr import label_maximum, train_logistic_regression, train_multinomial_logistic_regression

        family = self.getOrDefault("family")
        if family not in ("auto", "binomial", "multinomial"):
            raise ValueError(f"unknown LogisticRegression family {family!r}")
        vc = frame.column(self.getFeaturesCol())
        y = frame.column(self.getLabelCol())
        w = frame.column(self.getWeightCol()) if self.isSet("weightCol") else None
        kw = dict(weights=w, max_iter=self.getMaxIter(), tol=self.getTol(), reg_param=self.getRegParam(),
                  elastic_net=self.getElasticNetParam(), fit_intercept=self.getFitIntercept(),
                  standardization=self.getStandardization())
        if family != "multinomial":
            ymax = label_maximum(y)
            if family == "binomial" and ymax > 1:
                raise ValueError(f"family='binomial' needs labels in {{0, 1}}, the largest label is {ymax:g}")
            if family == "auto" and ymax > 1:
                family = "multinomial"
        if family == "multinomial":
            coef, intercepts, history = train_multinomial_logistic_regression(vc, y, **kw)
            m = LogisticRegressionModel(coefficientMatrix=coef, interceptVector=intercepts, uid=self.uid)
        else:
            coef, intercept, history = train_logistic_regression(vc, y, **kw)
            m = LogisticRegressionModel(coef, intercept, uid=self.uid)
        m._paramMap.update(self._paramMap)
        m.objectiveHistory = history
        return m


@register("org.apache.spark.ml.classification.LogisticRegressionModel")
class LogisticRegressionModel(_LRParams, ClassificationModelBase):
    """A binomial model holds one coefficient row and one intercept; a multinomial model holds
    ``numClasses`` rows (``coefficientMatrix`` [C, F], ``interceptVector`` [C]). For the latter
    ``rawPrediction`` is the ``C`` class scores of ``ops.sparse.score_csr`` (``nb_score``),
    ``probability`` their max-subtracted softmax and ``prediction`` the first argmax (``threshold``
    is ignored, as in Spark). A 2-row model also serves through the single-launch paths as the
    margin ``raw_1 - raw_0``, exactly as a binary ``NaiveBayesModel`` does."""
    _uid_prefix = "LogisticRegression"

    def __init__(self, coefficients=None, intercept: float = 0.0, coefficientMatrix=None, interceptVector=None,
                 **kw):
        super().__init__(**kw)
        if coefficientMatrix is not None:
            self._set_model(coefficientMatrix, interceptVector)
        else:
            self._set_model(np.asarray(coefficients if coefficients is not None else [], dtype=np.float64)[None, :],
                            [float(intercept)])
        self.objectiveHistory: list = []

    def _set_model(self, matrix, intercepts) -> None:
        self._W = np.ascontiguousarray(matrix, dtype=np.float64)
        if self._W.ndim != 2 or self._W.shape[0] < 1:
            raise ValueError("coefficientMatrix is [numClasses, numFeatures] (one row for a binomial model)")
        self._b = np.zeros(self._W.shape[0]) if intercepts is None else \
            np.ascontiguousarray(intercepts, dtype=np.float64).reshape(-1)
        if self._b.size != self._W.shape[0]:
            raise ValueError("interceptVector needs one entry per row of coefficientMatrix")
        self._scorer = self._class_scorer = None

    @property
    def isMultinomial(self) -> bool:  # noqa: N802
        return self._W.shape[0] > 1

    @property
    def numClasses(self) -> int:  # noqa: N802
        return int(self._W.shape[0]) if self.isMultinomial else 2

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return int(self._W.shape[1])

    @property
    def coefficientMatrix(self) -> np.ndarray:  # noqa: N802
        return self._W

    @property
    def interceptVector(self) -> np.ndarray:  # noqa: N802
        return self._b

    @property
    def coefficients(self) -> np.ndarray:
        if self.isMultinomial:
            raise ValueError("a multinomial model has no single coefficient vector: use coefficientMatrix")
        return self._W[0]

    @property
    def intercept(self) -> float:
        if self.isMultinomial:
            raise ValueError("a multinomial model has no single intercept: use interceptVector")
        return float(self._b[0])

    def class_scorer(self) -> ClassLinearScorer:
        """The rows as ``C`` linear class scores (``W`` feature-major); multinomial models only."""
        if not self.isMultinomial:
            raise ValueError("a binomial model scores one margin: use scorer()")
        if self._class_scorer is None:
            self._class_scorer = ClassLinearScorer(np.ascontiguousarray(self._W.T), self._b, exact=True)
        return self._class_scorer

    def scorer(self) -> LinearScorer:
        """The margin as one ``LinearScorer``; of a 2-row model ``raw_1 - raw_0`` (differences taken
        once in fp64)."""
        if self.numClasses != 2:
            raise ValueError(f"the single-launch and streaming paths score binary models only; this logistic "
                             f"regression model has {self.numClasses} classes (use transform / predictRaw)")
        if self._scorer is None:
            self._scorer = LinearScorer(self._W[1] - self._W[0], float(self._b[1] - self._b[0])) \
                if self.isMultinomial else LinearScorer(self.coefficients, self.intercept)
        return self._scorer

    def serving_scorer(self):
        return self.class_scorer() if self.numClasses > 2 else self.scorer()

    def postprocess(self, raw: torch.Tensor):
        if self.isMultinomial:
            if raw.shape[1] == 1:                    # the serving paths' margin raw_1 - raw_0
                if self.numClasses != 2:
                    raise ValueError("a margin describes a binary model")
                m = raw[:, 0]
                rp = torch.stack([torch.zeros_like(m), m], dim=1)
                prob = 1.0 / (1.0 + torch.exp(-torch.stack([-m, m], dim=1)))
                return rp, prob, _argmax_prediction(prob)
            if raw.shape[1] != self.numClasses:
                raise ValueError(f"expected [N, {self.numClasses}] class scores or an [N, 1] margin")
            e = torch.exp(raw - raw.max(dim=1, keepdim=True).values)
            prob = e / e.sum(dim=1, keepdim=True)
            return raw, prob, _argmax_prediction(prob)
        m = raw[:, 0]
        rp = torch.stack([-m, m], dim=1)
        prob = 1.0 / (1.0 + torch.exp(-rp))           # Spark raw2probability on [-m, m]
        pred = (prob[:, 1] > self.getThreshold()).to(torch.float64)
        return rp, prob, pred

    def contributions(self, features) -> VectorColumn:
        """Every row stores its own entries ``w_f * x_f``, then the intercept at ``numFeatures``."""
        if self.isMultinomial or self.getOrDefault("family") == "multinomial":
            raise NotImplementedError("contributions of multinomial logistic regression are not supported")
        vc = self._features_column(features)
        if vc.size != self.numFeatures:
            raise ValueError(f"features have size {vc.size}, model expects {self.numFeatures}")
        return _linear_contributions(vc, self.scorer().weights(vc.device), self.intercept, self.numFeatures)

    def postprocess_numpy(self, raw: np.ndarray):
        if self.isMultinomial and raw.shape[1] != 1:
            return super().postprocess_numpy(raw)
        p = np.exp(-raw[:, 0])
        np.add(p, 1.0, out=p)
        np.reciprocal(p, out=p)
        if self.isMultinomial:                       # first argmax of [1 - p, p]
            return (p > 1.0 - p).astype(np.float64), p
        return (p > self.getThreshold()).astype(np.float64), p

    def _score(self, vc: VectorColumn) -> torch.Tensor:
        from ..ops.sparse import score_csr

        return score_csr(vc, self.class_scorer() if self.isMultinomial else self.scorer())

    def _transform(self, frame: Frame) -> Frame:
        if not self.isMultinomial:
            return super()._transform(frame)
        return self.attach_outputs(frame, self._score(self._features_column(frame)))

    def predictRaw(self, features) -> DenseVector:  # noqa: N802
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self.postprocess(self._score(vc))[0][0].cpu().numpy())

    def predictProbability(self, features) -> DenseVector:  # noqa: N802
        if not self.isMultinomial:
            return super().predictProbability(features)
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self.postprocess(self._score(vc))[1][0].cpu().numpy())

    def predict(self, features) -> float:
        if not self.isMultinomial:
            return super().predict(features)
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return float(self.postprocess(self._score(vc))[2][0])

    def _metadata_extra(self):
        return None

    def _save_data(self, path) -> None:
        fields = [sf.Field.simple("numClasses", "integer"), sf.Field.simple("numFeatures", "integer"),
                  sf.Field.vector("interceptVector"), sf.Field.matrix("coefficientMatrix"),
                  sf.Field.simple("isMultinomial", "boolean")]
        if not self.isMultinomial:
            sf.write_data_parquet(path, fields, [
                {"numClasses": 2, "numFeatures": self.numFeatures, "interceptVector": sf.dense_vector([self.intercept]),
                 "coefficientMatrix": sf.sparse_matrix_row_major(self.coefficients[None, :]), "isMultinomial": False}])
            return
        # Spark's Matrix.compressed: the smaller of the dense and the row-major sparse form (12 bytes
        # per stored entry against 8 per cell); a -0.0 survives only the dense form
        W = self._W
        nnz = int(np.count_nonzero(W))
        sparse = 12 * nnz + 4 * (W.shape[0] + 1) < 8 * W.size and not bool(np.any(np.signbit(W) & (W == 0)))
        sf.write_data_parquet(path, fields, [
            {"numClasses": self.numClasses, "numFeatures": self.numFeatures,
             "interceptVector": sf.dense_vector(self._b),
             "coefficientMatrix": sf.sparse_matrix_row_major(W) if sparse else sf.dense_matrix(W),
             "isMultinomial": True}])

    def _load_data(self, path, md) -> None:
        row = sf.read_data_parquet(path).to_pylist()[0]
        coef = sf.decode_matrix(row["coefficientMatrix"]).astype(np.float64)
        icpt = sf.decode_vector(row["interceptVector"])
        if row.get("isMultinomial"):
            self._set_model(coef, icpt)
        else:
            self._set_model(coef[:1], [float(icpt[0])])
        self.objectiveHistory = []


# ============================================================================ trees
class _TreeParams(_PredictorParams):
    _params = [Param("maxDepth", "max tree depth", 5, int),
               Param("maxBins", "max bins for continuous features", 32, int),
               Param("minInstancesPerNode", "min rows per child", 1, int),
               Param("minWeightFractionPerNode", "min weight fraction per child", 0.0, float),
               Param("minInfoGain", "min info gain to split", 0.0, float),
               Param("maxMemoryInMB", "histogram memory budget", 256, int),
               Param("cacheNodeIds", "cache node ids", False, bool),
               Param("checkpointInterval", "checkpoint interval", 10, int),
               Param("impurity", "gini|entropy", "gini", str),
               Param("seed", "random seed", None, int, has_default=False),
               Param("leafCol", "leaf index column", "", str),
               Param("weightCol", "weight column", None, str, has_default=False)]

    def _default_hook(self) -> None:
        # Spark: seed default = hash of the class name
        self._defaultParamMap.setdefault("seed", _java_string_hash(type(self).__name__.replace("Model", "")))


def _java_string_hash(s: str) -> int:
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h - (1 << 32) if h >= (1 << 31) else h


class TreeClassificationModelBase(ClassificationModelBase):
    leaf_payload = "counts"

    def __init__(self, trees=None, num_features: int = 0, tree_weights=None, **kw):
        super().__init__(**kw)
        self._trees = list(trees or [])
        self._num_features = int(num_features)
        self._tree_weights = np.asarray(tree_weights if tree_weights is not None else np.ones(len(self._trees)))
        self._arrays: Optional[TreeArrays] = None

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return self._num_features

    @property
    def trees(self) -> list:
        return self._trees

    def scorer(self) -> TreeArrays:
        if self._arrays is None:
            self._arrays = ensemble_arrays(self._trees, self.leaf_payload, None, cmp_less=False)
        return self._arrays

    def paths(self):
        """TreeSHAP path table of class 1, cached with (and as long as) the scorer's arrays."""
        arrays = self.scorer()
        cached = self.__dict__.get("_paths")
        if cached is None or cached[0] is not arrays:
            cached = self._paths = (arrays, ensemble_paths(self._trees, self.leaf_payload, None, cmp_less=False))
        return cached[1]

    def contributions(self, features) -> VectorColumn:
        paths = self.paths()
        return self._tree_contributions(features, paths, paths.bias)

    def postprocess(self, raw: torch.Tensor):
        prob = _normalize(raw)
        return raw, prob, _argmax_prediction(prob)

    @property
    def featureImportances(self):  # noqa: N802
        from .linalg import SparseVector

        imp = feature_importances(self._trees, self._num_features)
        nz = np.nonzero(imp)[0]
        return SparseVector(self._num_features, nz, imp[nz])

    def _metadata_extra(self):
        return {"numFeatures": self._num_features, "numClasses": 2}


@register("org.apache.spark.ml.classification.DecisionTreeClassifier")
class DecisionTreeClassifier(_TreeParams, Estimator):
    _uid_prefix = "DecisionTreeClassifier"

    def _fit(self, frame: Frame):
        from ..models.tree import fit_forest

        res = fit_forest(frame.column(self.getFeaturesCol()), frame.column(self.getLabelCol()),
                         num_trees=1, max_depth=self.getMaxDepth(), max_bins=self.getMaxBins(),
                         min_instances=self.getMinInstancesPerNode(), min_info_gain=self.getMinInfoGain(),
                         bootstrap=False, feature_subset="all", seed=self.getSeed(), impurity=self.getImpurity())
        m = DecisionTreeClassificationModel(res.trees, res.num_features, uid=self.uid)
        m._paramMap.update(self._paramMap)
        return m


@register("org.apache.spark.ml.classification.DecisionTreeClassificationModel")
class DecisionTreeClassificationModel(_TreeParams, TreeClassificationModelBase):
    _uid_prefix = "DecisionTreeClassifier"
    leaf_payload = "counts"

    @property
    def depth(self) -> int:
        return self._trees[0].depth() if self._trees else 0

    @property
    def numNodes(self) -> int:  # noqa: N802
        return self._trees[0].compacted().num_nodes if self._trees else 0

    def _save_data(self, path) -> None:
        sf.write_data_parquet(path, NODE_FIELDS, self._trees[0].to_node_rows())

    def _load_data(self, path, md) -> None:
        rows = sf.read_data_parquet(path).to_pylist()
        self._trees = [Tree.from_node_rows(rows)]
        self._num_features = int(md.get("numFeatures", 0))
        self._tree_weights = np.ones(1)
        self._arrays = None


class _RFParams(_TreeParams):
    _params = [Param("numTrees", "number of trees", 20, int),
               Param("featureSubsetStrategy", "features per node", "auto", str),
               Param("subsamplingRate", "row subsampling rate", 1.0, float),
               Param("bootstrap", "bootstrap rows", True, bool)]


@register("org.apache.spark.ml.classification.RandomForestClassifier")
class RandomForestClassifier(_RFParams, Estimator):
    """``numWorkers`` (extension, not a Spark param): data-parallel rank processes for ``fit``
    (parallel/estimator_dp.py); never persisted, so saved stages stay loadable by Spark."""
    _uid_prefix = "RandomForestClassifier"
    _params = [Param("numWorkers", "data-parallel rank processes (extension)", 1, int)]
    _persist_defaults_only = ("numWorkers",)

    def _fit(self, frame: Frame):
        from ..models.tree import fit_forest
        from ..parallel import dist as D

        n = self.getNumTrees()
        kw = dict(num_trees=n, max_depth=self.getMaxDepth(), max_bins=self.getMaxBins(),
                  min_instances=self.getMinInstancesPerNode(), min_info_gain=self.getMinInfoGain(),
                  bootstrap=bool(self.getBootstrap()) and n > 1, feature_subset=self.getFeatureSubsetStrategy(),
                  seed=self.getSeed(), impurity=self.getImpurity(), subsampling_rate=self.getSubsamplingRate())
        X, y = frame.column(self.getFeaturesCol()), frame.column(self.getLabelCol())
        from ..parallel.estimator_dp import effective_workers

        from ..utils.config import default_device

        dev = default_device()
        nw = effective_workers(self.getOrDefault("numWorkers"), len(X), dev, nnz=X.nnz, kind="rf")
        if nw > 1 and not D.is_dist():
            from ..parallel.estimator_dp import fit_data_parallel

            (trees, nf), self.last_dp_report = fit_data_parallel("rf", X, y, None, kw, nw, device=dev)
        else:
            res = fit_forest(X, y, device=dev, **kw)
            trees, nf = res.trees, res.num_features
        m = RandomForestClassificationModel(trees, nf, uid=self.uid)
        m._paramMap.update({k: v for k, v in self._paramMap.items() if k != "numWorkers"})
        return m


@register("org.apache.spark.ml.classification.RandomForestClassificationModel")
class RandomForestClassificationModel(_RFParams, TreeClassificationModelBase):
    _uid_prefix = "RandomForestClassifier"
    leaf_payload = "normalized"

    @property
    def treeWeights(self) -> list:  # noqa: N802
        return [float(w) for w in self._tree_weights]

    def _metadata_extra(self):
        return {"numFeatures": self._num_features, "numClasses": 2, "numTrees": len(self._trees)}

    def _save_data(self, path) -> None:
        rows = []
        for t, tree in enumerate(self._trees):
            for r in tree.to_node_rows():
                rows.append({"treeID": t, "nodeData": r})
        sf.write_data_parquet(path, [sf.Field.simple("treeID", "integer"),
                                     sf.Field.struct("nodeData", NODE_FIELDS)], rows)
        params_json = sf.spark_json_dumps({"class": "org.apache.spark.ml.classification.DecisionTreeClassificationModel"})
        meta_rows = [{"treeID": t, "metadata": params_json, "weights": float(w)}
                     for t, w in enumerate(self._tree_weights)]
        sf.write_data_parquet(path, [sf.Field.simple("treeID", "integer"), sf.Field.simple("metadata", "string", True),
                                     sf.Field.simple("weights", "double")], meta_rows, subdir="treesMetadata")

    def _load_data(self, path, md) -> None:
        rows = sf.read_data_parquet(path).to_pylist()
        by_tree: dict = {}
        for r in rows:
            by_tree.setdefault(r["treeID"], []).append(r["nodeData"])
        self._trees = [Tree.from_node_rows(by_tree[k]) for k in sorted(by_tree)]
        try:
            meta = sf.read_data_parquet(path, "treesMetadata").to_pylist()
            w = {r["treeID"]: r["weights"] for r in meta}
            self._tree_weights = np.asarray([w.get(k, 1.0) for k in sorted(by_tree)])
        except FileNotFoundError:
            self._tree_weights = np.ones(len(self._trees))
        self._num_features = int(md.get("numFeatures", 0))
        self._arrays = None


# ============================================================================ naive Bayes
class _NBParams(_PredictorParams):
    _params = [Param("smoothing", "additive (Laplace / Lidstone) smoothing", 1.0, float),
               Param("modelType", "multinomial|bernoulli (complement and gaussian are not supported)",
                     "multinomial", str),
               Param("weightCol", "weight column", None, str, has_default=False),
               Param("thresholds", "per-class thresholds: the prediction is the first argmax of p_c / t_c",
                     None, list, has_default=False)]


@register("org.apache.spark.ml.classification.NaiveBayes")
class NaiveBayes(_NBParams, Estimator):
    """Spark's ``NaiveBayes`` (multinomial and Bernoulli) with an exact fixed-point fit
    (``models/nb.py``): host fits, device fits and every world size give the same model bits. Data
    parallelism is through the ambient process group, as for ``LogisticRegression``."""
    _uid_prefix = "NaiveBayes"

    def _fit(self, frame: Frame) -> "NaiveBayesModel":
        from ..models.nb import fit_naive_bayes

        w = frame.column(self.getWeightCol()) if self.isSet("weightCol") else None
        res = fit_naive_bayes(frame.column(self.getFeaturesCol()), frame.column(self.getLabelCol()), weights=w,
                              smoothing=self.getSmoothing(), model_type=self.getModelType())
        m = NaiveBayesModel(res["pi"], res["theta"], uid=self.uid)
        m._paramMap.update(self._paramMap)
        return m


@register("org.apache.spark.ml.classification.NaiveBayesModel")
class NaiveBayesModel(_NBParams, ClassificationModelBase):
    """``pi`` [C] class log-priors and ``theta`` [C, F] feature log-probabilities. ``rawPrediction`` is
    the ``C`` class scores of ``ops.sparse.score_csr`` (``nb_score``), ``probability`` Spark's
    ``raw2probability`` (subtract the row maximum, ``exp``, divide by the sum).

    A binary model also serves through the single-launch paths: ``scorer()`` is the margin
    ``raw_1 - raw_0`` as one ``LinearScorer``, and ``postprocess`` of a margin ``m`` [N, 1] gives
    ``probability = [sigma(-m), sigma(m)]`` and ``rawPrediction = [0, m]``: Spark's ``rawPrediction``
    minus the per-row constant ``raw_0`` (probabilities and predictions are those of the class
    scores up to rounding). Only the serving paths (``FusedPipeline.predict``, the agent, the
    streaming engine) see that form; ``transform`` gives Spark's ``rawPrediction``."""
    _uid_prefix = "NaiveBayes"

    def __init__(self, pi=None, theta=None, **kw):
        super().__init__(**kw)
        self._set_model(pi if pi is not None else np.zeros(0), theta if theta is not None else np.zeros((0, 0)))

    def _set_model(self, pi, theta) -> None:
        self.pi = np.asarray(pi, dtype=np.float64).reshape(-1)
        self.theta = np.asarray(theta, dtype=np.float64).reshape(self.pi.size, -1)
        self.sigma = np.zeros((0, 0))
        self._class_scorer = self._scorer = None

    @property
    def numClasses(self) -> int:  # noqa: N802
        return int(self.pi.size)

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return int(self.theta.shape[1])

    def class_scorer(self) -> ClassLinearScorer:
        if self._class_scorer is None:
            from ..models.nb import class_linear

            self._class_scorer = ClassLinearScorer(*class_linear(self.pi, self.theta, self.getModelType()), exact=True)
        return self._class_scorer

    def scorer(self) -> LinearScorer:
        """Binary models: the margin ``raw_1 - raw_0`` (differences taken once in fp64)."""
        if self.numClasses != 2:
            raise ValueError(f"the single-launch and streaming paths score binary models only; this Naive Bayes "
                             f"model has {self.numClasses} classes (use transform / predictRaw)")
        if self._scorer is None:
            cs = self.class_scorer()
            self._scorer = LinearScorer(cs.W[:, 1] - cs.W[:, 0], float(cs.b[1] - cs.b[0]))
        return self._scorer

    def serving_scorer(self):
        return self.class_scorer() if self.numClasses > 2 else self.scorer()

    def _thresholds(self, like: torch.Tensor) -> Optional[torch.Tensor]:
        if not self.isSet("thresholds"):
            return None
        t = torch.as_tensor(np.asarray(self.getThresholds(), dtype=np.float64)).to(like.device)
        if t.numel() != self.numClasses or bool((t < 0).any()) or int((t == 0).sum()) > 1:
            raise ValueError("thresholds needs one non-negative entry per class, at most one of them 0")
        return t

    def _predict_from(self, prob: torch.Tensor) -> torch.Tensor:
        t = self._thresholds(prob)
        if t is None:
            return _argmax_prediction(prob)
        zero = torch.where(prob == 0, torch.zeros_like(prob), torch.full_like(prob, float("inf")))
        scaled = torch.where(t == 0, zero, prob / torch.where(t == 0, torch.ones_like(t), t))
        return _argmax_prediction(scaled)

    def postprocess(self, raw: torch.Tensor):
        if raw.shape[1] == 1:                        # the serving paths' margin raw_1 - raw_0
            if self.numClasses != 2:
                raise ValueError("a margin describes a binary model")
            m = raw[:, 0]
            rp = torch.stack([torch.zeros_like(m), m], dim=1)
            prob = 1.0 / (1.0 + torch.exp(-torch.stack([-m, m], dim=1)))
            return rp, prob, self._predict_from(prob)
        if raw.shape[1] != self.numClasses:
            raise ValueError(f"expected [N, {self.numClasses}] class scores or an [N, 1] margin")
        e = torch.exp(raw - raw.max(dim=1, keepdim=True).values)
        prob = e / e.sum(dim=1, keepdim=True)
        return raw, prob, self._predict_from(prob)

    def postprocess_numpy(self, raw: np.ndarray):
        """Streaming hot path: margin [N, 1] -> (prediction [N], sigma(m) [N])."""
        if raw.shape[1] != 1 or self.isSet("thresholds"):
            return super().postprocess_numpy(raw)
        p = np.exp(-raw[:, 0])
        np.add(p, 1.0, out=p)
        np.reciprocal(p, out=p)
        return (p > 1.0 - p).astype(np.float64), p

    def _score(self, vc: VectorColumn) -> torch.Tensor:
        from ..ops.sparse import score_csr

        return score_csr(vc, self.class_scorer())

    def _transform(self, frame: Frame) -> Frame:
        return self.attach_outputs(frame, self._score(self._features_column(frame)))

    def predictRaw(self, features) -> DenseVector:  # noqa: N802
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self._score(vc)[0].cpu().numpy())

    def predictProbability(self, features) -> DenseVector:  # noqa: N802
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self.postprocess(self._score(vc))[1][0].cpu().numpy())

    def predict(self, features) -> float:
        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return float(self.postprocess(self._score(vc))[2][0])

    def contributions(self, features) -> VectorColumn:
        """Binary models: every row stores its own entries ``x_f * (W_f1 - W_f0)``, then the bias
        ``b_1 - b_0`` at ``numFeatures``; a row sums to the margin ``raw_1 - raw_0``."""
        vc = self._features_column(features)
        sc = self.scorer()
        w = sc.weights(vc.device)
        if vc.size > w.numel():
            w = torch.cat([w, torch.zeros(vc.size - w.numel(), dtype=torch.float64, device=w.device)])
        return _linear_contributions(vc, w, sc.b, vc.size)

    def _save_data(self, path) -> None:
        sf.write_data_parquet(path, [sf.Field.vector("pi"), sf.Field.matrix("theta"), sf.Field.matrix("sigma")],
                              [{"pi": sf.dense_vector(self.pi), "theta": sf.dense_matrix(self.theta),
                                "sigma": sf.dense_matrix(self.sigma)}])

    def _load_data(self, path, md) -> None:
        row = sf.read_data_parquet(path).to_pylist()[0]
        self._set_model(sf.decode_vector(row["pi"]), sf.decode_matrix(row["theta"]))


# ============================================================================ linear SVC
class _SVCParams(_PredictorParams):
    _params = [Param("weightCol", "weight column", None, str, has_default=False),
               Param("maxIter", "max iterations", 100, int),
               Param("regParam", "regularization", 0.0, float),
               Param("tol", "convergence tolerance", 1e-6, float),
               Param("fitIntercept", "fit an intercept", True, bool),
               Param("standardization", "standardize features", True, bool),
               Param("threshold", "threshold applied to the margin (rawPrediction[1])", 0.0, float),
               Param("aggregationDepth", "treeAggregate depth", 2, int),
               Param("maxBlockSizeInMB", "block size", 0.0, float)]

    _DEFAULT_ORDER = ("featuresCol", "labelCol", "predictionCol", "rawPredictionCol", "maxIter", "regParam", "tol",
                      "fitIntercept", "standardization", "threshold", "aggregationDepth", "maxBlockSizeInMB")

    @classmethod
    def params(cls) -> list:
        # Spark's LinearSVC is no probabilistic classifier: it has no probabilityCol
        return [p for p in super().params() if p.name != "probabilityCol"]

    def _default_hook(self) -> None:
        d = self._defaultParamMap
        self._defaultParamMap = {k: d[k] for k in self._DEFAULT_ORDER if k in d}


@register("org.apache.spark.ml.classification.LinearSVC")
class LinearSVC(_SVCParams, Estimator):
    """Spark's ``LinearSVC``: hinge loss with an L2 penalty on labels in {0, 1}, fitted by
    ``models/svm.py::train_linear_svc`` on the fused exact hinge pass. Data parallelism is through the
    ambient process group, as for ``LogisticRegression``."""
    _uid_prefix = "LinearSVC"

    def _fit(self, frame: Frame) -> "LinearSVCModel":
        from ..models.svm import train_linear_svc

        w = frame.column(self.getWeightCol()) if self.isSet("weightCol") else None
        coef, intercept, history = train_linear_svc(
            frame.column(self.getFeaturesCol()), frame.column(self.getLabelCol()), weights=w,
            max_iter=self.getMaxIter(), tol=self.getTol(), reg_param=self.getRegParam(),
            fit_intercept=self.getFitIntercept(), standardization=self.getStandardization())
        m = LinearSVCModel(coef, intercept, uid=self.uid)
        m._paramMap.update(self._paramMap)
        m.objectiveHistory = history
        return m


@register("org.apache.spark.ml.classification.LinearSVCModel")
class LinearSVCModel(_SVCParams, ClassificationModelBase):
    """One coefficient vector and one intercept. ``rawPrediction = [-m, m]`` with the margin
    ``m = coefficients . x + intercept``, ``prediction = 1.0`` iff ``m > threshold``; ``transform``
    adds no probability column, as Spark.

    The serving glue (``FusedPipeline.predict``, the agent, the streaming engine) expects a triple
    from ``postprocess``; its middle element is ``[sigma(-(m - threshold)), sigma(m - threshold)]``,
    which those paths report as ``confidence``. That is a monotone squashing of the margin, not a
    calibrated probability, and never a ``transform`` column: it is ``> 0.5`` exactly when the
    prediction is 1."""
    _uid_prefix = "LinearSVC"

    def __init__(self, coefficients=None, intercept: float = 0.0, **kw):
        super().__init__(**kw)
        self._set_model(coefficients if coefficients is not None else [], intercept)
        self.objectiveHistory: list = []

    def _set_model(self, coefficients, intercept) -> None:
        self._w = np.ascontiguousarray(coefficients, dtype=np.float64).reshape(-1)
        self._b = float(intercept)
        self._scorer = None

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return int(self._w.size)

    @property
    def coefficients(self) -> np.ndarray:
        return self._w

    @property
    def intercept(self) -> float:
        return self._b

    def scorer(self) -> LinearScorer:
        if self._scorer is None:
            self._scorer = LinearScorer(self._w, self._b)
        return self._scorer

    def postprocess(self, raw: torch.Tensor):
        m = raw[:, 0]
        rp = torch.stack([-m, m], dim=1)
        t = m - self.getThreshold()
        squashed = 1.0 / (1.0 + torch.exp(-torch.stack([-t, t], dim=1)))
        return rp, squashed, (m > self.getThreshold()).to(torch.float64)

    def attach_outputs(self, frame: Frame, raw: torch.Tensor) -> Frame:
        rp, _, pred = self.postprocess(raw)
        if self.getRawPredictionCol():
            frame = frame.withColumn(self.getRawPredictionCol(), rp)
        return frame.withColumn(self.getPredictionCol(), pred)

    def predictRaw(self, features) -> DenseVector:  # noqa: N802
        from ..ops.sparse import score_csr

        vc = VectorColumn.from_rows([features], size=self.numFeatures)
        return DenseVector(self.postprocess(score_csr(vc, self.scorer()))[0][0].cpu().numpy())

    def predictProbability(self, features) -> DenseVector:  # noqa: N802
        raise AttributeError("LinearSVCModel has no probability (Spark's LinearSVC is not probabilistic)")

    def contributions(self, features) -> VectorColumn:
        """Every row stores its own entries ``w_f * x_f``, then the intercept at ``numFeatures``; a row
        sums to the margin."""
        vc = self._features_column(features)
        if vc.size != self.numFeatures:
            raise ValueError(f"features have size {vc.size}, model expects {self.numFeatures}")
        return _linear_contributions(vc, self.scorer().weights(vc.device), self.intercept, self.numFeatures)

    def _save_data(self, path) -> None:
        sf.write_data_parquet(path, [sf.Field.vector("coefficients"), sf.Field.simple("intercept", "double")],
                              [{"coefficients": sf.dense_vector(self._w), "intercept": self._b}])

    def _load_data(self, path, md) -> None:
        row = sf.read_data_parquet(path).to_pylist()[0]
        self._set_model(sf.decode_vector(row["coefficients"]), float(row["intercept"]))
        self.objectiveHistory = []
