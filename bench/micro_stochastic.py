"""Cost of a GBDT boosting round under row and column subsampling: synthetic dialogues (HashingTF
2^18 -> IDF), depth 6, one GPU.

Reports ms per tree for each ``--subsample`` value and, with ``--columns``, for each column stage
at 0.5 and all three together (one JSON line per configuration, then a summary line).
A tree's time is the difference of two fits, (T(rounds) - T(short)) / (rounds - short), so the
quantisation of the features and the other per-fit setup cancel; fits are device-synchronised and
follow a warm-up fit.

``--pkg-root DIR`` imports the package from another checkout (``--subsample 1.0`` only there), to
alternate this tree with its parent commit in one GPU visit. ``--check-host`` grows 2 trees at
``--check-subsample`` on the device and on the host from the same rows and compares them bitwise.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--short", type=int, default=10)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--subsample", type=float, nargs="*", default=[1.0, 0.8, 0.5])
    ap.add_argument("--columns", action="store_true", help="also each colsample stage at 0.5, and all three")
    ap.add_argument("--check-host", action="store_true")
    ap.add_argument("--check-subsample", type=float, default=0.5)
    ap.add_argument("--pkg-root", default=os.path.dirname(HERE))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    assert args.rounds - args.short >= 40, "at least 40 trees per figure"
    sys.path.insert(0, args.pkg_root)
    sys.path.insert(1, os.path.join(args.pkg_root, "bench"))

    import torch

    from gbdt_train import build_features

    from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
    from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
    from fraud_detection_spark_kafka_llm_amd.models.warmup import warm_tree_kernels
    from fraud_detection_spark_kafka_llm_amd.ops.sparse import feature_order
    from fraud_detection_spark_kafka_llm_amd.parallel.affinity import bind_to_gpu

    dev = torch.device("cuda:0")
    bind_to_gpu(dev.index)
    warm_tree_kernels(dev, gbdt_depth=args.depth)
    F = 1 << 18
    indptr, idx, counts, y, _, _ = build_features(args.rows, dev)
    fo = feature_order(indptr, idx, counts, F)
    idf = torch.log((args.rows + 1.0) / (fo.df.double() + 1.0))
    train = VectorColumn.tfidf(F, indptr, idx, counts, idf, fo)

    def params(p, rounds):
        if isinstance(p, dict):
            kw = p
        else:
            kw = {} if p == 1.0 else {"subsample": p}     # (the parent commit has no such field)
        return GBDTParams(n_estimators=rounds, max_depth=args.depth, **kw)

    def fit(p, rounds, device=dev, data=train, labels=y):
        if device.type == "cuda":
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = fit_gbdt(data, labels, params(p, rounds), device=device)
        if device.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, res

    summary = {}
    configs = list(args.subsample)
    if args.columns:
        stages = ("colsample_bytree", "colsample_bylevel", "colsample_bynode")
        configs += [{k: 0.5} for k in stages] + [{k: 0.5 for k in stages}]
    for p in configs:
        fit(p, 2)                                             # allocator, code objects
        per_tree = []
        for _ in range(args.reps):
            t_short, _ = fit(p, args.short)
            t_long, res = fit(p, args.rounds)
            per_tree.append((t_long - t_short) / (args.rounds - args.short) * 1e3)
        rec = {"what": "ms_per_tree", "tag": args.tag, "config" if isinstance(p, dict) else "subsample": p,
               "rows": args.rows, "depth": args.depth, "trees": args.rounds - args.short, "ms": per_tree, "median_ms": statistics.median(per_tree),
               "nodes_last_tree": int(res.trees[-1].num_nodes), "deferred": getattr(res, "deferred", None)}
        print(json.dumps(rec), flush=True)
        summary["+".join(sorted(p)) if isinstance(p, dict) else str(p)] = rec["median_ms"]
    print(json.dumps({"what": "summary", "tag": args.tag, "rows": args.rows, "ms_per_tree": summary}), flush=True)

    if args.check_host:
        p = args.check_subsample
        if args.columns:
            p = {"subsample": p, "colsample_bytree": 0.5, "colsample_bylevel": 0.5, "colsample_bynode": 0.5}
        _, on_dev = fit(p, 2)
        cpu = torch.device("cpu")
        secs, on_host = fit(p, 2, cpu, train.to("cpu"), y.cpu())

        def sig(trees):
            return [(t.feature.tolist(), t.threshold.tolist(), t.stats.tolist()) for t in trees]

        same = sig(on_dev.trees) == sig(on_host.trees)
        print(json.dumps({"what": "device_equals_host", "rows": args.rows, "subsample": p, "trees": 2, "equal": same,
                          "host_fit_s": secs}), flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
