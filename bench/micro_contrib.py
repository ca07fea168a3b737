"""TreeSHAP contributions at the headline model shape: 100 trees x depth 6 on HashingTF 2^18 + IDF
features of 65,536 synthetic dialogues.

Times ``ops.sparse.tree_contributions`` on the device and on the host twin (16 threads), and
``score_csr`` on the same inputs for scale; checks that device and host agree bitwise. Prints one
JSON line per measurement and a final summary line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from fraud_detection_spark_kafka_llm_amd.data import synth
from fraud_detection_spark_kafka_llm_amd.ml import (IDF, Frame, HashingTF, Pipeline, StopWordsRemover, TextColumn,
                                                     Tokenizer)
from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import Tree
from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier, SparkXGBClassifierModel
from fraud_detection_spark_kafka_llm_amd.ops.sparse import contrib_limits, score_csr, tree_contributions


def timed(fn, reps: int, sync) -> list:
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def complete_trees(n_trees: int, depth: int, col, seed: int = 0) -> list:
    """Complete trees of ``depth`` (the worst case the trained model's early leaves fall short of):
    presence tests (threshold = half the smallest stored value) on features drawn by document
    frequency, random leaf values, covers halving towards the leaves with some jitter."""
    rng = np.random.default_rng(seed)
    idx = col.indices.cpu().numpy()
    val = col.values.cpu().numpy()
    df = np.bincount(idx, minlength=col.size).astype(np.float64)
    low = np.full(col.size, np.inf)
    np.minimum.at(low, idx, val)
    cand = np.flatnonzero((df > 0) & (low > 0))
    p = df[cand] / df[cand].sum()
    n = 2 ** (depth + 1) - 1
    inner = np.arange(n) < 2 ** depth - 1
    trees = []
    for _ in range(n_trees):
        f = np.where(inner, rng.choice(cand, n, p=p), -1).astype(np.int32)
        cover = np.zeros(n)
        cover[~inner] = rng.uniform(1.0, 3.0, int((~inner).sum()))
        for i in range(2 ** depth - 2, -1, -1):
            cover[i] = cover[2 * i + 1] + cover[2 * i + 2]
        kids = np.where(inner, 2 * np.arange(n) + 1, -1).astype(np.int32)
        stats = np.stack([np.where(inner, 0.0, rng.normal(0, 0.1, n)), cover], 1)
        trees.append(Tree(f, np.where(inner, 0.5 * low[np.maximum(f, 0)], 0.0), kids, np.where(inner, kids + 1, -1)
                          .astype(np.int32), stats, np.zeros(n), np.zeros(n), np.zeros(n, np.int64), stats[:, 0], 0))
    return trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complete", action="store_true",
                    help="random complete trees (2^depth leaves each) instead of a trained model")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pt, y = synth.generate(synth.SynthConfig(n=args.rows, seed=3))
    raw = TextColumn(pt.strings())
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})
    feats = Pipeline(stages=[Tokenizer(inputCol="clean_text", outputCol="words"),
                             StopWordsRemover(inputCol="words", outputCol="filtered_words"),
                             HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=1 << 18),
                             IDF(inputCol="raw_features", outputCol="features")]).fit(df).transform(df)
    col = feats.column("features")
    if args.complete:
        model = SparkXGBClassifierModel(complete_trees(args.trees, args.depth, col), col.size, 0.0)
    else:
        model = SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=args.trees,
                                   max_depth=args.depth).fit(feats)
    host_vc = col.to("cpu")
    host_vc = VectorColumn(col.size, host_vc.indptr, host_vc.indices, host_vc.values)
    dev_vc = host_vc.to(dev)
    paths, arrays = model.paths(), model.scorer()
    shape = {"rows": len(host_vc), "nnz": host_vc.nnz, "trees": len(model.trees), "paths": paths.num_paths,
             "elements": int(paths.pe_slot.size), "used_features": int(paths.features.size),
             "blocks": paths.num_blocks, "longest_slot": int(np.diff(paths.slot_ptr).max()), **contrib_limits()}
    print(json.dumps({"what": "shape", **shape}), flush=True)

    sync = torch.cuda.synchronize
    tree_contributions(dev_vc, paths)                       # warm-up: tables to the device, allocator
    t_dev = timed(lambda: tree_contributions(dev_vc, paths), args.reps, sync)
    print(json.dumps({"what": "tree_contributions_device", "ms": t_dev}), flush=True)
    score_csr(dev_vc, arrays)
    t_score = timed(lambda: score_csr(dev_vc, arrays), args.reps, sync)
    print(json.dumps({"what": "score_csr_device", "ms": t_score}), flush=True)
    got = tree_contributions(dev_vc, paths).cpu()
    t_host = []
    for _ in range(max(1, args.host_reps)):
        t0 = time.perf_counter()
        want = tree_contributions(host_vc, paths, threads=args.host_threads)
        t_host.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "tree_contributions_host", "threads": args.host_threads, "ms": t_host}), flush=True)
    same = bool(torch.equal(got, want))
    score = score_csr(host_vc, arrays)[:, 0]
    gap = float((got.sum(1) + paths.bias - score).abs().max())
    print(json.dumps({"what": "summary", "device_ms": statistics.median(t_dev),
                      "host_ms": statistics.median(t_host),
                      "score_csr_ms": statistics.median(t_score), "rows_per_tile": shape["rows_per_tile"],
                      "device_equals_host_bitwise": same, "efficiency_gap": gap}), flush=True)


if __name__ == "__main__":
    main()
