"""Cost of validation monitoring in a GBDT fit: 1M training rows of synthetic dialogues
(HashingTF 2^18 -> IDF) plus 100k and 1M validation rows, 100 rounds at depth 6 on one GPU.

Reports ms per round with validation off and with ``auc``, ``logloss`` and ``error`` (one JSON
line per configuration, then a summary line). A round's time is the difference of two fits,
(T(rounds) - T(short)) / (rounds - short), so quantisation and the other per-fit setup cancel.

``--only METRIC --val N`` runs a single monitored configuration: the form to put behind
``rocprofv3 --kernel-trace --stats --`` for the per-kernel times of ``tree_eval_update``, the sort
and the AUC kernels, and the launches per round (a run of its own: tracing changes the timings).
``--pkg-root DIR`` imports the package from another checkout (validation off only), to alternate
this tree with its parent commit in one GPU visit.
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
    ap.add_argument("--val", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--short", type=int, default=10)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="one metric (or 'off'): a single fit of --rounds rounds")
    ap.add_argument("--metrics", nargs="*", default=["off", "auc", "logloss", "error"])
    ap.add_argument("--pkg-root", default=os.path.dirname(HERE))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
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
    metrics = [args.only] if args.only else args.metrics
    val_sizes = args.val if any(m != "off" for m in metrics) else []
    vals = {}
    for n in val_sizes:
        # rows the training set does not hold, as raw TF-IDF values (what the model scorer reads)
        ip, ix, cn, yv, _, _ = build_features(n, dev, first_row=args.rows)
        vals[n] = (VectorColumn(F, ip, ix, cn.to(torch.float64) * idf[ix.long()]), yv.to(torch.float32), None)
        del cn

    def fit(metric, n_val, rounds):
        kw = {} if metric == "off" else dict(eval_set=vals[n_val], eval_metric=metric)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = fit_gbdt(train, y, GBDTParams(n_estimators=rounds, max_depth=args.depth), device=dev, **kw)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, res

    if args.only:
        n_val = val_sizes[0] if val_sizes else 0
        fit(args.only, n_val, 2)                                  # allocator, code objects
        secs, res = fit(args.only, n_val, args.rounds)
        print(json.dumps({"what": "single", "metric": args.only, "val_rows": n_val, "rounds": args.rounds,
                          "fit_s": secs, "deferred": getattr(res, "deferred", None)}), flush=True)
        return

    summary = {}
    for metric in metrics:
        for n_val in ([0] if metric == "off" else val_sizes):
            fit(metric, n_val, 2)
            per_round = []
            for _ in range(args.reps):
                t_short, _ = fit(metric, n_val, args.short)
                t_long, res = fit(metric, n_val, args.rounds)
                per_round.append((t_long - t_short) / (args.rounds - args.short) * 1e3)
            rec = {"what": "ms_per_round", "tag": args.tag, "metric": metric, "val_rows": n_val, "rows": args.rows,
                   "rounds": args.rounds, "ms": per_round, "median_ms": statistics.median(per_round),
                   "deferred": getattr(res, "deferred", None)}
            if metric != "off":
                rec["last"] = res.evals_result["validation"][metric][-1]
            print(json.dumps(rec), flush=True)
            summary[f"{metric}@{n_val}"] = rec["median_ms"]
    off = summary.get("off@0")
    print(json.dumps({"what": "summary", "tag": args.tag, "ms_per_round": summary,
                      "added_ms": {k: v - off for k, v in summary.items() if off is not None and k != "off@0"}}),
          flush=True)


if __name__ == "__main__":
    main()
