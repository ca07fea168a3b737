"""Naive Bayes on one GPU: the exact fixed-point class-sum pass (``nb_sums``), the C-class scorer
(``nb_score``) and a full ``fit_naive_bayes``, on synthetic dialogues through the fused featurizer
(HashingTF 2^18 term counts; ``--ngram 2`` for bigrams), against the formulations the project had
before: ``C`` calls of ``ops.sparse.spmv_t`` with ``r = w 1[y = c]``, ``C`` calls of ``spmv`` and the L2
``LogisticRegression`` fit.

JSON lines (times are medians of ``--reps`` by device events unless a host clock is named):
  * ``data``: rows, stored entries, the bytes one pass over the CSR, labels and weights must move;
  * ``sums``: ms of the ``nb_sums`` kernel at the default table and chunk, its bytes per second, ms of
    the ``C`` ``spmv_t`` calls (and of one), the spread (min .. max) of both, and whether the sums
    times 2^-k equal the ``spmv_t`` sums for these integer counts;
  * ``table``: the LDS table sweep (bytes of the table, hot slots, ms), 0 = every entry to a global atomic;
  * ``chunk``: the rows-per-workgroup sweep at the default table;
  * ``score``: ms of ``nb_score`` and of the ``C`` ``spmv`` calls, bit equality of the two;
  * ``fit``: host-clock seconds of ``fit_naive_bayes`` (maxima, hot set, pass, copy, finalize) and of
    ``train_logistic_regression`` with ``regParam`` 0.01 on the same features.

``--dry-run`` walks through every step once on the host at whatever size is given and measures nothing.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def event_ms(fn, reps, torch):
    """(median, min, max) ms by device events; (None, None, None) on the host."""
    if not torch.cuda.is_available():
        fn()
        return None, None, None
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def features(rows, ngram, dev, chunk=65536, seed=11):
    """Term-count CSR (float32) and labels of ``rows`` synthetic dialogues, chunk by chunk."""
    import torch

    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
    from fraud_detection_spark_kafka_llm_amd.ml.stopwords import ENGLISH
    from fraud_detection_spark_kafka_llm_amd.ops.text import FeatureSpec, featurize_score

    spec = FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=1 << 18, ngram=ngram)
    ptrs, idxs, vals, ys, off = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], [], 0
    for start in range(0, rows, chunk):
        n = min(chunk, rows - start)
        pt, y = synth.generate(synth.SynthConfig(n=n, seed=seed), device=dev, start=start)
        ip, ix, v = featurize_score(pt, spec, want_csr=True, device=dev).csr()
        ptrs.append(ip[1:] + off)
        idxs.append(ix)
        vals.append(v)
        ys.append(y.to(dev))
        off += int(ip[-1])
    vc = VectorColumn(spec.dim, torch.cat(ptrs), torch.cat(idxs).to(torch.int32), torch.cat(vals))
    return vc, torch.cat(ys).to(torch.float64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ngram", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lr-iters", type=int, default=100)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import torch

    from fraud_detection_spark_kafka_llm_amd.models.lr import train_logistic_regression
    from fraud_detection_spark_kafka_llm_amd.models.nb import class_linear, fit_naive_bayes
    from fraud_detection_spark_kafka_llm_amd.ops import native, sparse
    from fraud_detection_spark_kafka_llm_amd.ops.text import ClassLinearScorer

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    lim = sparse.nb_limits()
    vc, y = features(args.rows, args.ngram, dev)
    indptr, idx, val = vc.csr()
    N, nnz, F, C = len(vc), int(idx.numel()), vc.size, 2
    w = torch.ones(N, dtype=torch.float64, device=dev)
    moved = nnz * (4 + val.element_size()) + N * (8 + 8 + 8)
    print(json.dumps({"data": {"rows": N, "nnz": nnz, "features": F, "ngram": args.ngram, "pass_bytes": moved}}))

    k = sparse.nb_scale_exponent(float(val.max()), N)
    kw = sparse.nb_scale_exponent(1.0, N)
    out = torch.zeros(C * F + 2 * C + 1, dtype=torch.int64, device=dev)
    L = native.lib()

    def sums(table_bytes, chunk_rows=0):
        hot = sparse.nb_hot_set(indptr, idx, val, F, C, table_bytes) if table_bytes and dev.type == "cuda" else \
            torch.zeros(0, dtype=torch.int32, device=dev)
        slot_of, hot_feat = sparse.nb_hot_tables(hot, F, C) if dev.type == "cuda" else (None, None)

        def run():
            out.zero_()
            L.nb_sums(indptr, idx, val, y, w, C, F, k, kw, False, slot_of, hot_feat, out, chunk_rows, 0)
        return event_ms(run, reps, torch), int(hot.numel())

    r = [w * (y == c) for c in range(C)]
    g = [None] * C

    def parent():
        for c in range(C):
            g[c] = sparse.spmv_t(indptr, idx, val, r[c], F)

    (ms, lo, hi), slots = sums(lim["table_bytes"])
    S = out[:C * F].view(C, F).clone()
    p_ms, p_lo, p_hi = event_ms(parent, reps, torch)
    exact = bool(all(torch.equal(S[c].to(torch.float64) * 2.0 ** -k, g[c]) for c in range(C)))
    print(json.dumps({"sums": {"ms": ms, "min": lo, "max": hi, "hot_slots": slots, "k": k,
                               "gb_per_s": None if ms is None else moved / ms / 1e6,
                               "spmv_t_ms": p_ms, "spmv_t_min": p_lo, "spmv_t_max": p_hi,
                               "equals_spmv_t_sums": exact}}))
    table = []
    for kib in (0, 8, 16, 32, 48, 63):
        (t, a, b), h = sums(kib * 1024)
        table.append({"table_bytes": kib * 1024, "hot_slots": h, "ms": t, "min": a, "max": b})
    print(json.dumps({"table": table}))
    chunk = []
    for rows in (256, 512, 1024, 2048, 4096):
        (t, a, b), _ = sums(lim["table_bytes"], rows)
        chunk.append({"chunk_rows": rows, "ms": t, "min": a, "max": b})
    print(json.dumps({"chunk": chunk}))

    res = fit_naive_bayes(vc, y, device=dev)
    W, b = class_linear(res["pi"], res["theta"])
    scorer = ClassLinearScorer(W, b)
    Wc = [torch.from_numpy(W[:, c].copy()).to(dev) for c in range(C)]
    raw = [None]
    cols = [None] * C

    def score():
        raw[0] = sparse.score_csr(vc, scorer)

    def score_parent():
        for c in range(C):
            cols[c] = sparse.spmv(indptr, idx, val, Wc[c]) + float(b[c])

    s_ms, s_lo, s_hi = event_ms(score, reps, torch)
    sp_ms, sp_lo, sp_hi = event_ms(score_parent, reps, torch)
    same = bool(all(torch.equal(raw[0][:, c], cols[c]) for c in range(C)))
    print(json.dumps({"score": {"ms": s_ms, "min": s_lo, "max": s_hi, "spmv_ms": sp_ms, "spmv_min": sp_lo,
                                "spmv_max": sp_hi, "bitwise_equal": same}}))

    def clock(fn):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter() - t0

    nb_s = [clock(lambda: fit_naive_bayes(vc, y, device=dev)) for _ in range(min(reps, 3))]
    lr_hist = []
    lr_s = clock(lambda: lr_hist.append(train_logistic_regression(vc, y, max_iter=1 if args.dry_run else args.lr_iters,
                                                                  reg_param=0.01, device=dev)[2]))
    print(json.dumps({"fit": {"naive_bayes_s": None if args.dry_run else statistics.median(nb_s),
                              "naive_bayes_all": None if args.dry_run else nb_s,
                              "lr_s": None if args.dry_run else lr_s, "lr_evaluations": len(lr_hist[0])}}))


if __name__ == "__main__":
    main()
