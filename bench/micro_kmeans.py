"""KMeans on one GPU: the fused assign-and-accumulate pass (``km_step``), its assign-only mode, the
update (``km_centers``) and a full ``fit_kmeans``, on synthetic dialogues through the fused featurizer
(HashingTF 2^18 term counts; ``--ngram 2`` for bigrams), against the same statistics with torch ops
on the same device: the sparse-dense product for the dots, ``argmin``, and ``index_add_`` for the sums.

JSON lines (times are medians of ``--reps`` by device events unless a host clock is named):
  * ``data``: rows, stored entries, features;
  * ``step`` (one line per K in ``--ks``): ms of ``km_step`` with the sums and assign-only (with their
    spread), the bytes a call requests (the CSR once per tile of 8 centers and once for the sums, a
    64-byte line of ``CT`` per entry and tile, the row arrays, the zeroed ``S``) and the rate that makes,
    ms of ``km_centers``, ms of the torch formulation (or the error it raised), and whether the torch
    assignments agree (they may differ where two distances tie to rounding);
  * ``fit``: host-clock seconds and the iteration count of ``fit_kmeans`` (k-means||, ``--fit-k``).

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

from micro_nb import event_ms, features  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ngram", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--fit-k", type=int, default=8)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import torch

    from fraud_detection_spark_kafka_llm_amd.models import kmeans as KM
    from fraud_detection_spark_kafka_llm_amd.ops import sparse

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    vc, _ = features(args.rows, args.ngram, dev)
    indptr, idx, val = vc.csr()
    N, nnz, F = len(vc), int(idx.numel()), vc.size
    print(json.dumps({"data": {"rows": N, "nnz": nnz, "features": F, "ngram": args.ngram}}))

    norms = sparse.sim_norms(indptr, val)
    xnmax = float(norms.max()) ** 2
    k = sparse.nb_scale_exponent(float(val.abs().max()), N)
    kw = sparse.nb_scale_exponent(1.0, N)
    kc = sparse.nb_scale_exponent(8.0 * xnmax, N)
    row_of = torch.repeat_interleave(torch.arange(N, device=dev), indptr[1:] - indptr[:-1], output_size=nnz)
    v64 = val.to(torch.float64)
    xn = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, row_of, v64 * v64)
    X = torch.sparse_csr_tensor(indptr, idx.to(torch.int64), v64, size=(N, F))

    for K in args.ks:
        Kp = sparse.km_padded(K)
        pick = torch.linspace(0, N - 1, K).to(torch.int64)
        rows = KM._gather_rows(vc, pick, 0, dev)
        cs = KM._Centers.of_rows(rows, F, "euclidean", dev)
        CT, cn = cs.CT, cs.cn
        tables = sparse.hot_tables(indptr, idx, val, F, K)
        blk = [None]

        def step(sums=True):
            blk[0] = sparse.km_step(vc, CT, cn, K, "euclidean", k, kw, kc, hot=tables if sums else None, sums=sums,
                                    want_rows=True, check=False)

        ms, lo, hi = event_ms(step, reps, torch)
        full = blk[0]
        a_ms, a_lo, a_hi = event_ms(lambda: step(False), reps, torch)
        c_ms, _, _ = event_ms(lambda: sparse.km_centers(full.S, full.Wq, CT, K, k, kw, "euclidean"), reps, torch)
        tiles = Kp // 8
        entry = 4 + val.element_size()
        moved = nnz * entry * (tiles + 1) + nnz * 64 * tiles + N * (8 + 4 + 8) + 8 * K * F
        ref = {}

        def torch_step():
            dots = torch.sparse.mm(X, CT[:, :K].contiguous())
            d = torch.clamp(xn[:, None] + cn[None, :K] - 2.0 * dots, min=0.0)
            a = torch.argmin(d, dim=1)
            S = torch.zeros(K * F, dtype=torch.float64, device=dev)
            S.index_add_(0, a[row_of] * F + idx.to(torch.int64), v64)
            ref["assign"], ref["cnt"] = a, torch.bincount(a, minlength=K)

        try:
            t_ms, t_lo, t_hi = event_ms(torch_step, reps, torch)
            agree = float((ref["assign"].to(torch.int32) == full.assign).double().mean())
            t_err = None
        except RuntimeError as exc:                       # reported, never hidden: the yardstick is optional
            t_ms = t_lo = t_hi = agree = None
            t_err = str(exc).splitlines()[0]
        print(json.dumps({"step": {"K": K, "ms": ms, "min": lo, "max": hi, "assign_only_ms": a_ms,
                                   "assign_only_min": a_lo, "assign_only_max": a_hi, "centers_ms": c_ms,
                                   "hot_slots": 0 if tables[1] is None else int(tables[1].numel()),
                                   "bytes": moved, "gb_per_s": None if ms is None else moved / ms / 1e6,
                                   "torch_ms": t_ms, "torch_min": t_lo, "torch_max": t_hi, "torch_error": t_err,
                                   "torch_assign_agreement": agree, "flag": full.flag}}))

    def clock(fn):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    fits = [clock(lambda: KM.fit_kmeans(vc, args.fit_k, device=dev, max_iter=2 if args.dry_run else 20))
            for _ in range(min(reps, 3))]
    res = fits[0][1]
    print(json.dumps({"fit": {"k": res["k"], "seconds": None if args.dry_run else statistics.median(t for t, _ in fits),
                              "all": None if args.dry_run else [t for t, _ in fits], "iterations": res["num_iter"],
                              "cost": res["cost"], "sizes": [int(s) for s in res["sizes"]]}}))


if __name__ == "__main__":
    main()
