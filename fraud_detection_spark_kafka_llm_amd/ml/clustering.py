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


class _BisectingKMeansParams:
    _params = [Param("featuresCol", "features column name", "features", str),
               Param("predictionCol", "prediction column name", "prediction", str),
               Param("k", "desired number of leaf clusters (> 1)", 4, int),
               Param("maxIter", "max iterations of a level", 20, int),
               Param("minDivisibleClusterSize", "rows (>= 1.0) or share of the rows (< 1.0) a divisible cluster needs",
                     1.0, float),
               Param("distanceMeasure", "euclidean|cosine", "euclidean", str),
               Param("seed", "seed of every draw", 566573821, int),
               Param("weightCol", "weight column", None, str, has_default=False)]


class BisectingKMeansSummary:
    """``trainingCost`` (the sum of the leaves' costs), ``clusterSizes`` (leaves left to right), ``k``
    (their number), ``numIter`` (``maxIter``, as in Spark)."""

    def __init__(self, training_cost: float, cluster_sizes, k: int, num_iter: int):
        self.trainingCost = float(training_cost)
        self.clusterSizes = [int(s) for s in cluster_sizes]
        self.k = int(k)
        self.numIter = int(num_iter)


@register("org.apache.spark.ml.clustering.BisectingKMeans")
class BisectingKMeans(_BisectingKMeansParams, Estimator):
    """Spark's ``BisectingKMeans`` with an exact fixed-point fit (``models/bisecting.py``): host fits,
    device fits and every world size give the same tree bit for bit. Data parallelism is through the
    ambient process group, as for ``KMeans``."""
    _uid_prefix = "BisectingKMeans"

    def _fit(self, frame: Frame) -> "BisectingKMeansModel":
        from ..models.bisecting import fit_bisecting_kmeans

        w = frame.column(self.getWeightCol()) if self.isSet("weightCol") else None
        res = fit_bisecting_kmeans(frame.column(self.getFeaturesCol()), self.getK(), weights=w,
                                   max_iter=self.getMaxIter(), seed=self.getSeed(),
                                   min_divisible_cluster_size=self.getMinDivisibleClusterSize(),
                                   distance_measure=self.getDistanceMeasure())
        m = BisectingKMeansModel(res["index"], res["cnt"], res["center"], res["cost"], res["left"], uid=self.uid)
        m._paramMap.update(self._paramMap)
        m._summary = BisectingKMeansSummary(res["training_cost"], res["sizes"], res["k"], self.getMaxIter())
        return m


@register("org.apache.spark.ml.clustering.BisectingKMeansModel")
class BisectingKMeansModel(_BisectingKMeansParams, Model):
    """The tree as node arrays: ``index`` [m] (root 1, children ``2 i`` and ``2 i + 1``), ``size`` [m] rows,
    ``center`` [m, F], ``cost`` [m] and ``left`` [m] (the position of the left child, the right one
    follows it; -1 for a leaf). The leaves are the clusters, numbered left to right. ``transform`` adds
    an integer ``predictionCol``: a row descends the tree, as in Spark (one assign-only
    ``ops.sparse.km_group_step`` per depth; ties go to the left child); it does not take the nearest leaf.

    Persistence follows Spark 3.5 as far as it is known here: the ml metadata, and under ``data/``
    mllib's ``BisectingKMeansModel`` v3.0: a metadata JSON and one parquet row per node. The layout was
    written without a Spark-written model to compare with."""
    _uid_prefix = "BisectingKMeans"
    _summary: Optional[BisectingKMeansSummary] = None
    _MLLIB_CLASS = "org.apache.spark.mllib.clustering.BisectingKMeansModel"

    def __init__(self, index=None, size=None, center=None, cost=None, left=None, **kw):
        super().__init__(**kw)
        if index is None:
            index, size, center, cost, left = [1], [0], np.zeros((1, 0)), [0.0], [-1]
        self._set_model(index, size, center, cost, left)

    def _set_model(self, index, size, center, cost, left) -> None:
        from ..models.bisecting import leaf_order

        self.index = np.asarray(index, dtype=np.int64)
        self.size = np.asarray(size, dtype=np.int64)
        self.center = np.ascontiguousarray(np.asarray(center, dtype=np.float64))
        self.cost = np.asarray(cost, dtype=np.float64)
        self.left = np.asarray(left, dtype=np.int64)
        m = len(self.index)
        if self.center.ndim != 2 or not all(len(a) == m for a in (self.size, self.center, self.cost, self.left)):
            raise ValueError("index, size, cost and left hold one entry per node, center is [nodes, F]")
        self.leaves = leaf_order(self.index, self.left)

    def clusterCenters(self) -> list:  # noqa: N802
        return [self.center[p].copy() for p in self.leaves]

    @property
    def numFeatures(self) -> int:  # noqa: N802
        return int(self.center.shape[1])

    @property
    def hasSummary(self) -> bool:  # noqa: N802
        return self._summary is not None

    @property
    def summary(self) -> BisectingKMeansSummary:
        if self._summary is None:
            raise RuntimeError("no training summary: the model was loaded, not fitted")
        return self._summary

    def computeCost(self) -> float:  # noqa: N802
        """The sum of the leaves' training costs."""
        import math

        return math.fsum(self.cost[p] for p in self.leaves)

    def _assign(self, vc: VectorColumn):
        from ..models.bisecting import predict_bisecting

        return predict_bisecting(vc, self.index, self.center, self.left, self.getDistanceMeasure())

    def _transform(self, frame: Frame) -> Frame:
        vc = frame.column(self.getFeaturesCol())
        if not isinstance(vc, VectorColumn):
            vc = VectorColumn.from_rows(list(vc), size=self.numFeatures)
        return frame.withColumn(self.getPredictionCol(), self._assign(vc))

    def predict(self, features) -> int:
        return int(self._assign(VectorColumn.from_rows([features], size=self.numFeatures))[0])

    def _height(self, p: int) -> float:
        """mllib's height of a node: the largest distance from its center to a child's, 0 for a leaf."""
        if self.left[p] < 0:
            return 0.0
        a = self.center[p]
        out = 0.0
        for c in (self.left[p], self.left[p] + 1):
            b = self.center[c]
            d = 1.0 - float(a @ b) if self.getDistanceMeasure() == "cosine" else float(np.sqrt(((a - b) ** 2).sum()))
            out = max(out, d)
        return out

    def _save_data(self, path) -> None:
        from pathlib import Path

        data = Path(path) / "data"
        md = {"class": self._MLLIB_CLASS, "version": "3.0", "rootId": 1, "distanceMeasure": self.getDistanceMeasure(),
              "trainingCost": sf.JDouble(self.computeCost())}
        sf.write_file_with_crc(data / "metadata" / "part-00000", (sf.spark_json_dumps(md) + "\n").encode("utf-8"))
        sf.mark_success(data / "metadata")
        fields = [sf.Field.simple("index", "integer"), sf.Field.simple("size", "long"), sf.Field.vector("center"),
                  sf.Field.simple("norm", "double"), sf.Field.simple("cost", "double"), sf.Field.simple("height", "double"),
                  sf.Field.array("children", "integer")]
        rows = []
        for p in range(len(self.index)):
            kids = [] if self.left[p] < 0 else [int(self.index[self.left[p]]), int(self.index[self.left[p] + 1])]
            rows.append({"index": int(self.index[p]), "size": int(self.size[p]), "center": sf.dense_vector(self.center[p]),
                         "norm": float(np.sqrt((self.center[p] ** 2).sum())), "cost": float(self.cost[p]),
                         "height": self._height(p), "children": kids})
        sf.write_data_parquet(data, fields, rows)

    def _load_data(self, path, md) -> None:
        from pathlib import Path

        rows = {int(r["index"]): r for r in sf.read_data_parquet(Path(path) / "data").to_pylist()}
        order, queue = [], [1]                             # root first, then the pairs of every level by node index
        while queue:
            order += queue
            queue = [c for i in queue for c in rows[i]["children"]]
        pos = {i: p for p, i in enumerate(order)}
        left = [pos[rows[i]["children"][0]] if rows[i]["children"] else -1 for i in order]
        self._set_model(order, [rows[i]["size"] for i in order],
                        np.stack([sf.decode_vector(rows[i]["center"]) for i in order]), [rows[i]["cost"] for i in order],
                        left)
