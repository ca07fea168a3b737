"""Spark-ML-compatible API (pyspark.ml surface used by the reference)."""
from .base import Estimator, Model, Param, Params, Pipeline, PipelineModel, Transformer
from .classification import (DecisionTreeClassificationModel, DecisionTreeClassifier, LinearSVC, LinearSVCModel,
                             LogisticRegression, LogisticRegressionModel, NaiveBayes, NaiveBayesModel,
                             RandomForestClassificationModel, RandomForestClassifier)
from .clustering import (BisectingKMeans, BisectingKMeansModel, BisectingKMeansSummary, KMeans, KMeansModel,
                         KMeansSummary)
from .evaluation import ClusteringEvaluator
from .feature import (IDF, CountVectorizer, CountVectorizerModel, HashingTF, IDFModel, NGram, StopWordsRemover,
                      Tokenizer)
from .frame import Frame, Row, TextColumn, TokenColumn
from .fused import FusedPipeline
from .linalg import DenseVector, SparseVector, VectorColumn, Vectors
