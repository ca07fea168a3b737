"""Similar-case retrieval on one GPU: the batched exact top-k (``ops.sparse.topk_cosine`` behind
``serve.similar.HistoricalIndex.query``) against the single-query path it complements
(``ClassificationAgent.find_similar_historical_cases``, called once per dialogue), on synthetic
dialogues through a HashingTF 2^18 -> IDF pipeline.

JSON lines:
  * ``data``: rows, stored entries and bytes of the historical CSR;
  * ``topk``: ms of one ``topk_cosine`` call for Q featurized queries (device events, median of
    ``--reps``), the logical corpus bytes it streams (corpus bytes x query tiles) per second, and
    whether its rows equal the single-query path's on the first queries;
  * ``query``: ms of ``HistoricalIndex.query`` (featurize + top-k + the copy of the result to the
    host) by a host clock around the call, which ends in that copy;
  * ``parent``: ms per ``find_similar_historical_cases`` call (host clock, each call ends in a device
    to host copy), measured on at most ``--parent-calls`` of the Q dialogues, and the time of Q
    sequential calls (``measured`` when all Q ran, else ``extrapolated`` from the per-call median);
  * ``sweep``: ``topk`` at Q = 64 for every ``queries_per_pass``.

``--dry-run`` walks through every step once on the host at whatever size is given and measures
nothing (times print as null).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def event_ms(fn, reps, torch):
    if not torch.cuda.is_available():
        fn()
        return None
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def make_agent(dev, features, workdir):
    """A HashingTF -> IDF -> logistic-regression pipeline fitted on a few synthetic dialogues."""
    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml import (IDF, Frame, HashingTF, LogisticRegression, Pipeline,
                                                         StopWordsRemover, TextColumn, Tokenizer)
    from fraud_detection_spark_kafka_llm_amd.serve.agent import ClassificationAgent
    from fraud_detection_spark_kafka_llm_amd.serve.llm import StubLLM

    pt, y = synth.generate(synth.SynthConfig(n=2000, seed=3))
    raw = TextColumn(pt.strings())
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})
    model = Pipeline(stages=[Tokenizer(inputCol="clean_text", outputCol="words"),
                             StopWordsRemover(inputCol="words", outputCol="filtered_words"),
                             HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=features),
                             IDF(inputCol="raw_features", outputCol="features"),
                             LogisticRegression(featuresCol="features", labelCol="labels", maxIter=5)]).fit(df)
    path = os.path.join(workdir, "model")
    model.save(path)
    return ClassificationAgent(path, llm=StubLLM(), device=dev)


def historical_vectors(agent, rows, chunk=65536, seed=11):
    """TF-IDF CSR of ``rows`` synthetic dialogues by the agent's fused featurizer, chunk by chunk
    (what ``HistoricalIndex`` does with a frame's strings, without holding the strings)."""
    import torch

    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
    from fraud_detection_spark_kafka_llm_amd.ops.text import featurize_score

    fp, dev = agent.fused, agent.device
    idf = fp.idf.idf_tensor(dev) if fp.idf is not None else None
    ptrs, idxs, vals, off = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], 0
    for start in range(0, rows, chunk):
        pt, _ = synth.generate(synth.SynthConfig(n=min(chunk, rows - start), seed=seed), device=dev, start=start)
        ip, ix, v = featurize_score(pt, fp.spec(True), idf=idf, want_csr=True, device=dev).csr()
        ptrs.append(ip[1:] + off)
        idxs.append(ix.to(torch.int32))
        vals.append(v.to(torch.float64))
        off += int(ip[-1])
    return VectorColumn(fp.dim, torch.cat(ptrs), torch.cat(idxs), torch.cat(vals))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--features", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-calls", type=int, default=64)
    ap.add_argument("--dry-run", action="store_true", help="one pass on the host, nothing is measured")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))

    import numpy as np
    import torch

    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn
    from fraud_detection_spark_kafka_llm_amd.ops.sparse import sim_limits, topk_cosine
    from fraud_detection_spark_kafka_llm_amd.serve.similar import HistoricalIndex, featurize

    if not args.dry_run and not torch.cuda.is_available():
        raise SystemExit("micro_similar.py measures on a HIP device; none is visible")
    dev = torch.device("cpu" if args.dry_run else "cuda:0")
    sync = (lambda: None) if args.dry_run else (lambda: torch.cuda.synchronize(dev))
    lim = sim_limits()
    qmax = max(args.queries)
    with tempfile.TemporaryDirectory() as tmp:
        agent = make_agent(dev, args.features, tmp)
    texts = synth.generate(synth.SynthConfig(n=qmax, seed=77))[0].strings()        # the new dialogues
    for rows in args.rows:
        t0 = time.perf_counter()
        vc = historical_vectors(agent, rows)
        sync()
        ip, ix, v = vc.csr()
        nnz = int(ix.numel())
        corpus_bytes = nnz * (4 + 8) + (rows + 1) * 8 + rows * 8
        base = {"tag": args.tag, "rows": rows, "nnz": nnz, "k": args.k}
        print(json.dumps({"what": "data", **base, "corpus_bytes": corpus_bytes,
                          "build_s": None if args.dry_run else time.perf_counter() - t0}), flush=True)
        frame = Frame({"dialogue": TextColumn(["-"] * rows), "row": np.arange(rows)})
        hist = HistoricalIndex.from_vectors(agent.fused, frame, vc)
        # the single-query path over the same arrays: its index as the method builds it (norms by index_add_)
        agent.historical_data = frame
        norms = torch.zeros(rows, dtype=torch.float64, device=dev)
        norms.index_add_(0, torch.repeat_interleave(torch.arange(rows, device=dev), ip[1:] - ip[:-1]), v * v)
        agent._hist_index = (vc, torch.sqrt(norms))
        for nq in args.queries:
            qvc = featurize(agent.fused, texts[:nq])
            run = (lambda qpp=0: topk_cosine(hist.index, qvc, args.k, queries_per_pass=qpp))
            got_rows, _ = run()
            sync()
            reps = args.reps if rows * nq <= 10 ** 9 else 1
            ms = event_ms(run, reps, torch)
            tiles = -(-nq // lim["queries_per_pass"])
            check = min(nq, 8)
            same = sum(int([r["row"] for r in agent.find_similar_historical_cases(texts[i], args.k)] ==
                           got_rows[i].tolist()) for i in range(check))
            print(json.dumps({"what": "topk", **base, "queries": nq, "ms": ms, "reps": reps, "query_tiles": tiles,
                              "streamed_gbytes_per_s": None if ms is None else corpus_bytes * tiles / (ms * 1e-3) / 1e9,
                              "rows_equal_parent": f"{same}/{check}"}), flush=True)
            hist.query(texts[:nq], args.k)
            t = time.perf_counter()
            for _ in range(reps):
                hist.query(texts[:nq], args.k)
            print(json.dumps({"what": "query", **base, "queries": nq,
                              "ms": None if args.dry_run else (time.perf_counter() - t) / reps * 1e3}), flush=True)
            calls = min(nq, args.parent_calls)
            per = []
            for i in range(calls):
                t = time.perf_counter()
                agent.find_similar_historical_cases(texts[i], args.k)
                per.append((time.perf_counter() - t) * 1e3)
            med = statistics.median(per)
            print(json.dumps({"what": "parent", **base, "queries": nq, "calls_timed": calls,
                              "ms_per_call": None if args.dry_run else med,
                              "ms_all": None if args.dry_run else (sum(per) if calls == nq else med * nq),
                              "ms_all_is": "measured" if calls == nq else "extrapolated"}), flush=True)
            if nq == 64:
                for qpp in range(1, lim["queries_per_pass"] + 1):
                    run(qpp)
                    print(json.dumps({"what": "sweep", **base, "queries": nq, "queries_per_pass": qpp,
                                      "ms": event_ms(lambda: run(qpp), reps, torch)}), flush=True)
        del hist, vc, frame
        agent.historical_data = None


if __name__ == "__main__":
    main()
