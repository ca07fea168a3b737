"""Linear SVC on one GPU: the fused exact hinge evaluation (``svc_eval``) on synthetic dialogues
through the fused featurizer (HashingTF 2^18 term counts; ``--ngram 2`` for bigrams), at ``beta = 0``
(every row is active) and at the fitted model (most rows are inside the margin), against the
formulation of the same quantities the project had before: ``spmv`` for the margins, torch
element-wise ops for the hinge terms and the sums, ``spmv_t`` for the gradient (what
``train_logistic_regression.fg`` does for the logistic loss).

JSON lines (times are medians of ``--reps`` by device events unless a host clock is named):
  * ``data``: rows, stored entries, features;
  * ``fit``: host-clock seconds, iterations and evaluations of a ``--fit-iters``-iteration
    ``train_linear_svc`` with ``regParam`` 0.01, unstandardised, and the active-row share at its end;
  * ``eval`` (one line per point, ``at`` = ``zero`` or ``fitted``): ms of ``svc_eval`` (zeroing its block
    included) at the default table and chunk, ms of the parent formulation, the spread (min .. max) of
    both, their ratio, the active-row share, and the largest difference of the two gradients relative
    to the largest gradient entry;
  * ``table`` (one line per point): the LDS table sweep (bytes of the table, hot slots, ms), 0 = every
    entry to a global atomic.

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
    ap.add_argument("--fit-iters", type=int, default=100)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import torch

    from fraud_detection_spark_kafka_llm_amd.models import svm as SVM
    from fraud_detection_spark_kafka_llm_amd.ops import sparse

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    vc, y = features(args.rows, args.ngram, dev)
    indptr, idx, val = vc.csr()
    N, nnz, F = len(vc), int(idx.numel()), vc.size
    print(json.dumps({"data": {"rows": N, "nnz": nnz, "features": F, "ngram": args.ngram}}), flush=True)
    k, kl = sparse.mlr_scale_exponents(1.0, float(val.abs().max()), N)
    s = 2.0 * y - 1.0

    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    coef, intercept, hist = SVM.train_linear_svc(vc, y, max_iter=1 if args.dry_run else args.fit_iters, reg_param=0.01,
                                                 standardization=False, device=dev)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    print(json.dumps({"fit": {"seconds": None if args.dry_run else fit_s, "iterations": len(hist) - 1,
                              "evaluations": SVM.SVC_STATS["evaluations"], "objective": hist[-1],
                              "active_share": SVM.SVC_STATS["active_share"], "k": k, "kl": kl}}), flush=True)

    points = {"zero": (torch.zeros(F, dtype=torch.float64, device=dev), 0.0),
              "fitted": (torch.from_numpy(coef).to(dev), float(intercept))}
    for at, (xs, b) in points.items():
        keep = {}

        def fused(table_bytes):
            hot = sparse.nb_hot_set(indptr, idx, val, F, 1, table_bytes) if table_bytes and dev.type == "cuda" else \
                torch.zeros(0, dtype=torch.int32, device=dev)
            tables = sparse.nb_hot_tables(hot, F, 1) if dev.type == "cuda" else (None, None)

            def run():
                keep["block"] = sparse.svc_eval(indptr, idx, val, xs, b, y, None, k, kl, tables, check_extents=False)
            return event_ms(run, reps, torch), int(hot.numel())

        def parent():
            m = sparse.spmv(indptr, idx, val, xs) + b
            z = 1.0 - s * m
            r = torch.where(z > 0, -s, torch.zeros_like(s))
            keep["loss"] = torch.clamp(z, min=0).sum()
            keep["gb"] = r.sum()
            keep["G"] = sparse.spmv_t(indptr, idx, val, r, F)

        (ms, lo, hi), slots = fused(sparse.svc_limits()["table_bytes"])
        p_ms, p_lo, p_hi = event_ms(parent, reps, torch)
        G = keep["block"].Gq.to(torch.float64) * 2.0 ** -k
        gap = float((G - keep["G"]).abs().max() / keep["G"].abs().max().clamp(min=1e-300))
        loss_gap = abs(keep["block"].lossq * 2.0 ** -kl - float(keep["loss"])) / max(float(keep["loss"]), 1e-300)
        print(json.dumps({"eval": {"at": at, "ms": ms, "min": lo, "max": hi, "hot_slots": slots,
                                   "active_share": keep["block"].nact / N,
                                   "parent_ms": p_ms, "parent_min": p_lo, "parent_max": p_hi,
                                   "parent_over_fused": None if ms is None else p_ms / ms,
                                   "gradient_gap_rel": gap, "loss_gap_rel": loss_gap}}), flush=True)
        table = []
        for kib in (0, 8, 16, 32, 48, 63):
            (t, a, c_), h = fused(kib * 1024)
            table.append({"table_bytes": kib * 1024, "hot_slots": h, "ms": t, "min": a, "max": c_})
        print(json.dumps({"table": {"at": at, "sweep": table}}), flush=True)


if __name__ == "__main__":
    main()
