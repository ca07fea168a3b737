"""pyspark.ml.clustering: ``KMeans`` / ``KMeansModel`` on the exact fixed-point trainer
(``models/kmeans.py``). Persistence follows Spark 3.5: one parquet row per center,
``clusterIdx: integer, clusterCenter: vector``."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ..io import spark_format as sf
from .base import Estimator, Model, Param, register
from .frame import Frame
from .linalg import VectorColumn


class _KMeansParams:
    _params = [Param("featuresCol", "features column name", "features", str),
               Param("predictionCol", "prediction column name", "prediction", str),
               Param("k", "number of clusters (> 1)", 2, int),
               Param("maxIter", "max iterations", 20, int),
               Param("tol", "a center that moved no further has converged", 1e-4, float),
               Param("initMode", "random|k-means||", "k-means||", str),
               Param("initSteps", "rounds of k-means||", 2, int),
               Param("distanceMeasure", "euclidean|cosine", "euclidean", str),
               Param("seed", "seed of every draw", -1689246527, int),
               Param("weightCol", "weight column", None, str, has_default=False)]


class KMeansSummary:
    """``trainingCost`` (the weighted cost of the final centers), ``clusterSizes``, ``numIter``, ``k``."""

    def __init__(self, training_cost: float, cluster_sizes, num_iter: int, k: int):
        self.trainingCost = float(training_cost)
        self.clusterSizes = [int(s) for s in cluster_sizes]
        self.numIter = int(num_iter)
        self.k = int(k)


@register("org.apache.spark.ml.clustering.KMeans")
class KMeans(_KMeansParams, Estimator):
    """Spark's ``KMeans`` with an exact fixed-point fit: host fits, device fits and every world size
    give the same centers bit for bit. Data parallelism is through the ambient process group, as for
    ``NaiveBayes``."""
    _uid_prefix = "KMeans"

    def _fit(self, frame: Frame) -> "KMeansModel":
        from ..models.kmeans import fit_kmeans

        w = frame.column(self.getWeightCol()) if self.isSet("weightCol") else None
        res = fit_kmeans(frame.column(self.getFeaturesCol()), self.getK(), weights=w, max_iter=self.getMaxIter(),
                         tol=self.getTol(), init_mode=self.getInitMode(), init_steps=self.getInitSteps(),
                         distance_measure=self.getDistanceMeasure(), seed=self.getSeed())
        m = KMeansModel(res["centers"], uid=self.uid)
        m._paramMap.update(self._paramMap)
        m._summary = KMeansSummary(res["cost"], res["sizes"], res["num_iter"], res["k"])
        return m


@register("org.apache.spark.ml.clustering.KMeansModel")
class KMeansModel(_KMeansParams, Model):
    """``centers`` [K, F]. ``transform`` adds an integer ``predictionCol``: the assign-only pass of
    ``ops.sparse.km_step``, the smallest index among the nearest centers."""
    _uid_prefix = "KMeans"
    _summary: Optional[KMeansSummary] = None

    def __init__(self, centers=None, **kw):
        super().__init__(**kw)
        self._set_model(centers if centers is not None else np.zeros((0, 0)))

    def _set_model(self, centers) -> None:
        self.centers = np.ascontiguousarray(np.asarray(centers, dtype=np.float64))
        if self.centers.ndim != 2:
            raise ValueError("centers is [K, F]")

    def clusterCenters(self) -> list:  # noqa: N802
        return [c.copy() for c in self.centers]

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return int(self.centers.shape[1])

    @property
    def hasSummary(self) -> bool:  # noqa: N802
        return self._summary is not None

    @property
    def summary(self) -> KMeansSummary:
        if self._summary is None:
            raise RuntimeError("no training summary: the model was loaded, not fitted")
        return self._summary

    def _assign(self, vc: VectorColumn):
        from ..models.kmeans import predict_kmeans

        return predict_kmeans(vc, self.centers, self.getDistanceMeasure())

    def _transform(self, frame: Frame) -> Frame:
        vc = frame.column(self.getFeaturesCol())
        if not isinstance(vc, VectorColumn):
            vc = VectorColumn.from_rows(list(vc), size=self.numFeatures)
        return frame.withColumn(self.getPredictionCol(), self._assign(vc))

    def predict(self, features) -> int:
        return int(self._assign(VectorColumn.from_rows([features], size=self.numFeatures))[0])

    def _save_data(self, path) -> None:
        sf.write_data_parquet(path, [sf.Field.simple("clusterIdx", "integer"), sf.Field.vector("clusterCenter")],
                              [{"clusterIdx": i, "clusterCenter": sf.dense_vector(c)} for i, c in enumerate(self.centers)])

    def _load_data(self, path, md) -> None:
        rows = sorted(sf.read_data_parquet(path).to_pylist(), key=lambda r: r["clusterIdx"])
        self._set_model(np.stack([sf.decode_vector(r["clusterCenter"]) for r in rows]))
