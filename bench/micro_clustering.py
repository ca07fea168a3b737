"""BisectingKMeans and the silhouette on one GPU: the candidate-given Lloyd step (``km_group_step``), the
silhouette pass (``sil_score``), one ``ClusteringEvaluator`` evaluation and one ``BisectingKMeans`` fit, on
synthetic dialogues through the fused featurizer (HashingTF 2^18 term counts), against the same
statistics with torch ops on the same device (the yardstick of ``micro_kmeans.py``: the sparse-dense
product for the dots, gathers of a row's candidates, ``index_add_`` for the sums).

JSON lines (times are medians of ``--reps`` by device events unless a host clock is named, each with
its spread):
  * ``data``: rows, stored entries, features;
  * ``group_step`` (one line per pair count in ``--pairs`` and share of live rows in ``--live``): ms of
    ``km_group_step`` with ``W = 2`` and the sums, and assign-only; the share ``1 / 32`` marks every other
    row skipped (``group = -1``); ms of the torch formulation over the live rows;
  * ``km_step_k2``: ms of ``km_step`` at ``K = 2`` on the same rows, the step a ``W = 2`` pass of one pair
    replaces;
  * ``sil_score`` (one line per K in ``--ks``): ms of the pass and of the torch formulation;
  * ``evaluate``: host-clock seconds of ``silhouette`` (both passes and the host arithmetic between);
  * ``fit``: host-clock seconds of ``fit_bisecting_kmeans`` (``--fit-k``), the passes of every level and the
    share of them at levels deeper than the first, where most rows of a pass are skipped.

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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--live", type=int, nargs="+", default=[1, 32], help="one row in this many is live")
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--fit-k", type=int, default=8)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import torch

    from fraud_detection_spark_kafka_llm_amd.models import bisecting as BK
    from fraud_detection_spark_kafka_llm_amd.models import kmeans as KM
    from fraud_detection_spark_kafka_llm_amd.models.silhouette import silhouette
    from fraud_detection_spark_kafka_llm_amd.ops import sparse

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    vc, _ = features(args.rows, 1, dev)
    indptr, idx, val = vc.csr()
    N, nnz, F = len(vc), int(idx.numel()), vc.size
    print(json.dumps({"data": {"rows": N, "nnz": nnz, "features": F}}))

    norms = sparse.sim_norms(indptr, val)
    xnmax = float(norms.max()) ** 2
    k = sparse.nb_scale_exponent(float(val.abs().max()), N)
    kw = sparse.nb_scale_exponent(1.0, N)
    kc = sparse.nb_scale_exponent(8.0 * xnmax, N)
    ks = sparse.nb_scale_exponent(2.0, N)
    lens = indptr[1:] - indptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(N, device=dev), lens, output_size=nnz)
    v64 = val.to(torch.float64)
    xn = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, row_of, v64 * v64)
    X = torch.sparse_csr_tensor(indptr, idx.to(torch.int64), v64, size=(N, F))
    rows_i = torch.arange(N, device=dev)

    def centers_of(K):
        pick = torch.linspace(0, N - 1, K).to(torch.int64)
        cs = KM._Centers.of_rows(KM._gather_rows(vc, pick, 0, dev), F, "euclidean", dev)
        return cs.CT, cs.cn

    def timed(fn):
        try:
            return event_ms(fn, reps, torch) + (None,)
        except RuntimeError as exc:                       # reported, never hidden: the yardstick is optional
            return None, None, None, str(exc).splitlines()[0]

    for G in args.pairs:
        K = max(2, 2 * G)
        CT, cn = centers_of(K)
        tables = sparse.hot_tables(indptr, idx, val, F, K)
        for live in args.live:
            group = (rows_i % G).to(torch.int32)
            if live > 1:
                group = torch.where(rows_i % live == 0, group, torch.full_like(group, -1))
            blk = [None]

            def step(sums=True):
                blk[0] = sparse.km_group_step(vc, group, 2, G, CT, cn, "euclidean", k, kw, kc,
                                              hot=tables if sums else None, sums=sums, want_rows=True, check=False)

            ms, lo, hi = event_ms(step, reps, torch)
            full = blk[0]
            a_ms, a_lo, a_hi = event_ms(lambda: step(False), reps, torch)
            keep = group >= 0
            Xl = torch.sparse_csr_tensor(*_take(torch, indptr, idx, v64, keep, lens), size=(int(keep.sum()), F))
            g64, live_entries = group[keep].to(torch.int64), keep[row_of]

            def torch_step():
                dots = torch.sparse.mm(Xl, CT[:, :K].contiguous())
                d0 = torch.clamp(xn[keep] + cn[2 * g64] - 2.0 * dots.gather(1, (2 * g64)[:, None])[:, 0], min=0.0)
                d1 = torch.clamp(xn[keep] + cn[2 * g64 + 1] - 2.0 * dots.gather(1, (2 * g64 + 1)[:, None])[:, 0], min=0.0)
                a = torch.full((N,), -1, dtype=torch.int64, device=dev)
                a[keep] = 2 * g64 + (d1 < d0)
                S = torch.zeros(K * F, dtype=torch.float64, device=dev)
                S.index_add_(0, a[row_of][live_entries] * F + idx[live_entries].to(torch.int64), v64[live_entries])
                torch.bincount(a[keep], minlength=K)

            t_ms, t_lo, t_hi, t_err = timed(torch_step)
            print(json.dumps({"group_step": {"pairs": G, "live_one_in": live, "live_rows": int(keep.sum()), "ms": ms,
                                             "min": lo, "max": hi, "assign_only_ms": a_ms, "assign_only_min": a_lo,
                                             "assign_only_max": a_hi,
                                             "hot_slots": 0 if tables[1] is None else int(tables[1].numel()),
                                             "torch_ms": t_ms, "torch_min": t_lo, "torch_max": t_hi,
                                             "torch_error": t_err, "flag": full.flag}}))

    CT, cn = centers_of(2)
    tables = sparse.hot_tables(indptr, idx, val, F, 2)
    ms, lo, hi = event_ms(lambda: sparse.km_step(vc, CT, cn, 2, "euclidean", k, kw, kc, hot=tables, want_rows=True,
                                                 check=False), reps, torch)
    print(json.dumps({"km_step_k2": {"ms": ms, "min": lo, "max": hi}}))

    for K in args.ks:
        Kp = sparse.km_padded(K)
        labels = (rows_i % K).to(torch.int32)
        blk = sparse.km_group_step(vc, labels, 1, K, torch.zeros((F, Kp), dtype=torch.float64, device=dev),
                                   torch.zeros(Kp, dtype=torch.float64, device=dev), "euclidean", k, kw, kc, check=False)
        MT, _, _ = sparse.km_centers(blk.S, blk.Wq, torch.zeros((F, Kp), dtype=torch.float64, device=dev), K, k, kw,
                                     "euclidean")
        nw, psi = (torch.zeros(Kp, dtype=torch.float64, device=dev) for _ in range(2))
        nw[:K] = torch.ldexp(blk.Wq.to(torch.float64), torch.tensor(-kw, device=dev))
        psi[:K] = torch.ldexp(blk.costq.to(torch.float64), torch.tensor(-kc, device=dev)) / nw[:K]
        cnt = torch.zeros(Kp, dtype=torch.int32, device=dev)
        cnt[:K] = blk.cnt.to(torch.int32)
        out = [None]

        def sil():
            out[0] = sparse.sil_score(vc, labels, K, MT, psi, nw, cnt, "euclidean", ks, kw, want_rows=True, check=False)

        ms, lo, hi = event_ms(sil, reps, torch)
        l64 = labels.to(torch.int64)

        def torch_sil():
            D = xn[:, None] + psi[None, :K] - 2.0 * torch.sparse.mm(X, MT[:, :K].contiguous())
            own = D.gather(1, l64[:, None])[:, 0] * nw[l64] / (nw[l64] - 1.0)
            nb = D.scatter(1, l64[:, None], float("inf")).min(dim=1).values
            s = torch.where(own < nb, 1.0 - own / nb, torch.where(own > nb, nb / own - 1.0, torch.zeros_like(own)))
            s.sum()

        t_ms, t_lo, t_hi, t_err = timed(torch_sil)
        print(json.dumps({"sil_score": {"K": K, "ms": ms, "min": lo, "max": hi, "torch_ms": t_ms, "torch_min": t_lo,
                                        "torch_max": t_hi, "torch_error": t_err, "flag": out[0].flag,
                                        "value": out[0].silq / max(out[0].wq, 1) * 2.0 ** (kw - ks)}}))

    def clock(fn):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    labels = (rows_i % 8).to(torch.int32)
    evals = [clock(lambda: silhouette(vc, labels, None, "squaredEuclidean", device=dev)) for _ in range(min(reps, 3))]
    print(json.dumps({"evaluate": {"k": 8, "seconds": None if args.dry_run else statistics.median(t for t, _ in evals),
                                   "all": None if args.dry_run else [t for t, _ in evals], "value": evals[0][1]["value"]}}))
    fits = [clock(lambda: BK.fit_bisecting_kmeans(vc, args.fit_k, device=dev, max_iter=2 if args.dry_run else 20))
            for _ in range(min(reps, 3))]
    res = fits[0][1]
    passes = res["level_passes"]
    print(json.dumps({"fit": {"k": res["k"], "seconds": None if args.dry_run else statistics.median(t for t, _ in fits),
                              "all": None if args.dry_run else [t for t, _ in fits], "level_passes": passes,
                              "deep_pass_share": sum(passes[1:]) / max(sum(passes), 1), "cost": res["training_cost"],
                              "sizes": [int(s) for s in res["sizes"]]}}))


def _take(torch, indptr, idx, v64, keep, lens):
    """The CSR of the rows ``keep``."""
    n = lens[keep]
    ptr = torch.zeros(int(keep.sum()) + 1, dtype=torch.int64, device=indptr.device)
    torch.cumsum(n, 0, out=ptr[1:])
    entries = torch.repeat_interleave(keep, lens)
    return ptr, idx[entries].to(torch.int64), v64[entries]


if __name__ == "__main__":
    main()
