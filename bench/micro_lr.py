"""Logistic-regression training on one GPU: the L-BFGS (L2) route against the elastic-net OWL-QN
route on synthetic dialogues (default 1M rows, HashingTF 2^18 -> IDF; ``--ngram 2`` for bigrams).

Three kinds of JSON lines:
  * ``evaluation``: ms per function evaluation of both routes on the L2 problem (alpha = 0), where
    both are defined: the op sequence of the L-BFGS route's ``fg()`` (one SpMV, the torch
    element-wise ops and sums, the transposed SpMV) against ``OwlqnEvaluation`` (the fused
    kernels), alternating, timed with device events and no host read inside the window;
  * ``kernel``: ms of ``lr_forward``, ``lr_reduce``, ``lr_owlqn_step``, ``lr_pseudo_grad`` and the two
    SpMVs on their own (device events over ``--reps`` launches), with the forward kernel's bytes/s
    over the bytes it has to read and write;
  * ``fit``: seconds of a whole fit of both routes, iterations, and the model's non-zero count.

``--only l2|enet`` runs a single fit: the form to put behind ``rocprofv3 --kernel-trace --stats --``
for the per-kernel times (a run of its own: tracing changes the timings). ``--dry-run`` walks through
every step once on the host at whatever size is given and measures nothing (times print as null).
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def build_tfidf(rows, dev, num_features, ngram, chunk=250_000, seed=11):
    """Synthetic dialogues -> fused featurizer (chunked) -> one fp64 TF-IDF CSR and the labels."""
    import torch

    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml.stopwords import ENGLISH
    from fraud_detection_spark_kafka_llm_amd.ops import text as T

    spec = T.FeatureSpec(clean=True, stopwords=list(ENGLISH), num_features=num_features, ngram=ngram)
    ptrs, idxs, cnts, ys, off = [torch.zeros(1, dtype=torch.int64, device=dev)], [], [], [], 0
    for start in range(0, rows, chunk):
        n = min(chunk, rows - start)
        pt, yc = synth.generate(synth.SynthConfig(n=n, seed=seed), device=dev, start=start)
        ip, ix, v = T.featurize_score(pt, spec, want_csr=True, device=dev).csr()
        ptrs.append(ip[1:] + off)
        idxs.append(ix)
        cnts.append(v.to(torch.float64))
        ys.append(yc.to(torch.float64))
        off += int(ip[-1])
    indptr, idx, cnt = torch.cat(ptrs), torch.cat(idxs).to(torch.int32), torch.cat(cnts)
    df = torch.bincount(idx.long(), minlength=num_features)
    idf = torch.log((rows + 1.0) / (df.double() + 1.0))
    return indptr, idx, cnt * idf[idx.long()], torch.cat(ys)


def event_ms(fn, reps, torch):
    """Median ms of ``fn()`` over ``reps`` calls, each between two device events."""
    if not torch.cuda.is_available():           # --dry-run: call once, report no time
        fn()
        return None, []
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=1 << 18)
    ap.add_argument("--ngram", type=int, default=1)
    ap.add_argument("--reg", type=float, default=0.01)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--only", default="", choices=["", "l2", "enet"])
    ap.add_argument("--dry-run", action="store_true", help="one pass on the host, nothing is measured")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))

    import torch

    from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
    from fraud_detection_spark_kafka_llm_amd.models import lr as LR
    from fraud_detection_spark_kafka_llm_amd.ops import native
    from fraud_detection_spark_kafka_llm_amd.ops.sparse import spmv
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import Collectives

    if not args.dry_run and not torch.cuda.is_available():
        raise SystemExit("micro_lr.py measures on a HIP device; none is visible")
    dev = torch.device("cpu" if args.dry_run else "cuda:0")
    sync = (lambda: None) if args.dry_run else (lambda: torch.cuda.synchronize(dev))
    C = native.lib()
    F = args.features
    t0 = time.perf_counter()
    indptr, idx, val, y = build_tfidf(args.rows, dev, F, args.ngram)
    sync()
    n, nnz = args.rows, int(idx.numel())
    base = {"tag": args.tag, "rows": n, "features": F, "ngram": args.ngram, "nnz": nnz}
    print(json.dumps({"what": "data", **base, "build_s": None if args.dry_run else time.perf_counter() - t0}), flush=True)
    vc = VectorColumn(F, indptr, idx, val)

    def fit(alpha):
        sync()
        t = time.perf_counter()
        coef, b, hist = LR.train_logistic_regression(vc, y, max_iter=args.max_iter, reg_param=args.reg,
                                                     elastic_net=alpha, device=dev)
        sync()
        rec = {"what": "fit", **base, "route": "enet" if alpha > 0 else "l2", "reg": args.reg, "alpha": alpha,
               "fit_s": None if args.dry_run else time.perf_counter() - t, "iterations": len(hist) - 1, "objective": hist[-1],
               "nonzero": int((coef != 0).sum())}
        if alpha > 0:
            rec.update(LR.OWLQN_STATS)
        return rec

    if args.only:
        alpha = args.alpha if args.only == "enet" else 0.0
        fit(alpha)                                                     # code objects, allocator
        print(json.dumps(fit(alpha)), flush=True)
        return

    # ---------------------------------------------------------------- one evaluation, both routes, L2 problem
    w = torch.ones(n, dtype=torch.float64, device=dev)
    wsum = float(n)
    t_csr = LR.transpose_csr(indptr, idx, val, F)
    scale = torch.ones(F, dtype=torch.float64, device=dev)
    theta = torch.zeros(F + 1, dtype=torch.float64, device=dev)
    theta[:F] = torch.randn(F, dtype=torch.float64, device=dev) * 1e-3

    def parent_fg():                # the ops of the L-BFGS route's fg(), without its host read
        beta, b = theta[:F], theta[F]
        m = spmv(indptr, idx, val, scale * beta) + b
        loss_i = torch.clamp(m, min=0) - m * y + torch.log1p(torch.exp(-torch.abs(m)))
        r = w * (torch.sigmoid(m) - y)
        parts = torch.cat([(w * loss_i).sum().reshape(1), r.sum().reshape(1), spmv(*t_csr, r)])
        loss = parts[0] / wsum + 0.5 * args.reg * torch.dot(beta, beta)
        g = torch.empty_like(theta)
        g[:F] = scale * parts[2:] / wsum + args.reg * beta
        g[F] = parts[1] / wsum
        return loss, g

    evaluation = LR.OwlqnEvaluation((indptr, idx, val), t_csr, y, w, wsum, scale, Collectives(), 0.0, args.reg, True)
    zero = torch.zeros_like(theta)
    xi = torch.sign(theta)

    def fused():
        return evaluation(theta, zero, xi, zero, 1.0)

    (x_new, _, g_new, _, _, _), packed = fused()
    loss_old, g_old = parent_fg()
    same = {"objective_diff": abs(float(packed[0]) - float(loss_old)),
            "grad_max_diff": float((g_new - g_old).abs().max()), "x_kept": bool(torch.equal(x_new, theta))}
    old_ms, new_ms = [], []
    for _ in range(args.reps):                                         # alternate the two routes
        old_ms.append(event_ms(parent_fg, 1, torch)[0])
        new_ms.append(event_ms(fused, 1, torch)[0])
    med = (lambda v: None) if args.dry_run else statistics.median
    print(json.dumps({"what": "evaluation", **base, "parent_fg_ms": med(old_ms), "fused_ms": med(new_ms), "parent_all": old_ms, "fused_all": new_ms, **same}),
          flush=True)

    # ---------------------------------------------------------------- the kernels on their own
    per = int(C.lr_limits()["rows_per_partial"])
    groups = int(C.lr_param_groups(F + 1))
    fwd_p = torch.empty((2, (n + per - 1) // per), dtype=torch.float64, device=dev)
    step_p = torch.empty((3, groups), dtype=torch.float64, device=dev)
    grad_p = torch.empty((1, groups), dtype=torch.float64, device=dev)
    r = torch.empty(n, dtype=torch.float64, device=dev)
    xs, x2 = torch.empty(F, dtype=torch.float64, device=dev), torch.empty_like(theta)
    out2, out3 = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    parts = torch.randn(F + 2, dtype=torch.float64, device=dev)
    gg, pp, xx = torch.empty_like(theta), torch.empty_like(theta), torch.empty_like(theta)
    margins = torch.empty(n, dtype=torch.float64, device=dev)
    kernels = {
        "lr_owlqn_step": lambda: C.lr_owlqn_step(theta, zero, xi, zero, scale, 1.0, x2, xs, step_p, 0),
        "lr_forward": lambda: C.lr_forward(indptr, idx, val, xs, x2[F:], y, w, r, None, None, fwd_p, 0),
        "lr_reduce(forward)": lambda: C.lr_reduce(fwd_p, out2),
        "lr_reduce(step)": lambda: C.lr_reduce(step_p, out3),
        "lr_pseudo_grad": lambda: C.lr_pseudo_grad(parts, scale, theta, wsum, 0.0, args.reg, True, gg, pp, xx, grad_p, 0),
        "spmv": lambda: C.spmv(indptr, idx, val, xs, margins, 0),
        "spmv(transposed)": lambda: C.spmv(*t_csr, r, parts[2:], 0),
    }
    # bytes lr_forward has to move: the CSR, labels and weights in; residuals and partials out
    fwd_bytes = nnz * (4 + 8) + (n + 1) * 8 + 2 * n * 8 + n * 8 + fwd_p.numel() * 8
    for name, fn in kernels.items():
        fn()
        ms, every = event_ms(fn, args.reps, torch)
        rec = {"what": "kernel", **base, "kernel": name, "ms": ms, "all": every}
        if name == "lr_forward" and ms:
            rec.update(bytes=fwd_bytes, gbytes_per_s=fwd_bytes / (ms * 1e-3) / 1e9)
        print(json.dumps(rec), flush=True)

    # ---------------------------------------------------------------- whole fits
    fit(0.0), fit(args.alpha)
    for _ in range(args.fit_reps):
        for alpha in (0.0, args.alpha):
            print(json.dumps(fit(alpha)), flush=True)


if __name__ == "__main__":
    main()
