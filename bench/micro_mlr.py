"""Multinomial logistic regression on one GPU: the fused fixed-point evaluation (``mlr_eval``) on
synthetic dialogues through the fused featurizer (HashingTF 2^18 term counts; ``--ngram 2`` for
bigrams) at ``C`` = 2, 3 and 8 classes, against the formulation of the same quantities the project had
before: ``nb_score`` for the margins, torch for the softmax, the residuals and the loss, and ``C``
calls of ``ops.sparse.spmv_t`` for the gradient.

JSON lines, one set per ``C`` (times are medians of ``--reps`` by device events unless a host clock is named):
  * ``data``: rows, stored entries, features;
  * ``eval``: ms of ``mlr_eval`` (zeroing its block included) at the default table and chunk, ms of the
    parent formulation, the spread (min .. max) of both, their ratio, and the largest difference of the
    two gradients relative to the largest gradient entry;
  * ``table``: the LDS table sweep (bytes of the table, hot slots, ms), 0 = every entry to a global atomic;
  * ``fit``: host-clock seconds and evaluations of a ``--fit-iters``-iteration
    ``train_multinomial_logistic_regression`` with ``regParam`` 0.01, unstandardised.

``--dry-run`` walks through every step once on the host at whatever size is given and measures nothing.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from micro_nb import event_ms, features  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ngram", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 3, 8])
    ap.add_argument("--fit-iters", type=int, default=30)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import torch

    from fraud_detection_spark_kafka_llm_amd.models import lr as LR
    from fraud_detection_spark_kafka_llm_amd.ops import sparse
    from fraud_detection_spark_kafka_llm_amd.ops.text import ClassLinearScorer

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    lim = sparse.mlr_limits()
    vc, y2 = features(args.rows, args.ngram, dev)
    indptr, idx, val = vc.csr()
    N, nnz, F = len(vc), int(idx.numel()), vc.size
    print(json.dumps({"data": {"rows": N, "nnz": nnz, "features": F, "ngram": args.ngram}}), flush=True)
    k, kl = sparse.mlr_scale_exponents(1.0, float(val.abs().max()), N)
    gen = torch.Generator().manual_seed(5)

    for C in args.classes:
        # the scam label in the lowest bit, the row number above it: every class has rows of both kinds
        y = ((y2.long() + 2 * (torch.arange(N, device=dev) % ((C + 1) // 2))) % C).to(torch.float64)
        XS = (torch.randn((F, C), generator=gen, dtype=torch.float64) * 0.05).to(dev)
        b = (torch.randn(C, generator=gen, dtype=torch.float64) * 0.1).to(dev)
        scorer = ClassLinearScorer(XS.cpu().numpy(), b.cpu().numpy())
        onehot = torch.nn.functional.one_hot(y.long(), C).to(torch.float64)
        keep = {}

        def fused(table_bytes):
            hot = sparse.nb_hot_set(indptr, idx, val, F, C, table_bytes) if table_bytes and dev.type == "cuda" else \
                torch.zeros(0, dtype=torch.int32, device=dev)
            tables = sparse.nb_hot_tables(hot, F, C) if dev.type == "cuda" else (None, None)

            def run():
                keep["block"] = sparse.mlr_eval(indptr, idx, val, XS, b, y, None, k, kl, tables, check_extents=False)
            return event_ms(run, reps, torch), int(hot.numel())

        def parent():
            m = sparse.score_csr(vc, scorer)
            mx = m.max(dim=1, keepdim=True).values
            e = torch.exp(m - mx)
            S = e.sum(dim=1, keepdim=True)
            R = (e / S - onehot).contiguous()
            keep["loss"] = ((mx - (m * onehot).sum(dim=1, keepdim=True)) + torch.log(S)).sum()
            keep["G"] = torch.stack([sparse.spmv_t(indptr, idx, val, R[:, c].contiguous(), F) for c in range(C)], dim=1)
            keep["gb"] = R.sum(dim=0)

        (ms, lo, hi), slots = fused(lim["table_bytes"])
        p_ms, p_lo, p_hi = event_ms(parent, reps, torch)
        G = keep["block"].Gq.to(torch.float64) * 2.0 ** -k
        gap = float((G - keep["G"]).abs().max() / keep["G"].abs().max())
        loss_gap = abs(keep["block"].lossq * 2.0 ** -kl - float(keep["loss"])) / float(keep["loss"])
        print(json.dumps({"eval": {"C": C, "ms": ms, "min": lo, "max": hi, "hot_slots": slots, "k": k, "kl": kl,
                                   "parent_ms": p_ms, "parent_min": p_lo, "parent_max": p_hi,
                                   "parent_over_fused": None if ms is None else p_ms / ms,
                                   "gradient_gap_rel": gap, "loss_gap_rel": loss_gap}}), flush=True)
        table = []
        for kib in (0, 8, 16, 32, 48):
            (t, a, c_), h = fused(kib * 1024)
            table.append({"table_bytes": kib * 1024, "hot_slots": h, "ms": t, "min": a, "max": c_})
        print(json.dumps({"table": {"C": C, "sweep": table}}), flush=True)

        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = LR.train_multinomial_logistic_regression(vc, y, max_iter=1 if args.dry_run else args.fit_iters,
                                                        reg_param=0.01, standardization=False, device=dev)[2]
        if dev.type == "cuda":
            torch.cuda.synchronize()
        fit_s = time.perf_counter() - t0
        print(json.dumps({"fit": {"C": C, "seconds": None if args.dry_run else fit_s, "iterations": len(hist) - 1,
                                  "evaluations": LR.MLR_STATS["evaluations"], "objective": hist[-1]}}), flush=True)


if __name__ == "__main__":
    main()
