"""Multi-class gradient boosting (``multi:softprob``) on one GPU: the two kernels and the trainer on
synthetic dialogues through the fused featurizer (HashingTF 2^18 term counts) at ``C`` = 2, 3 and 8.

JSON lines, one set per ``C`` (times are medians of ``--reps`` by device events unless a host clock is named):
  * ``data``: rows, stored entries, features;
  * ``grad``: ms of ``softprob_grad`` and bytes per second over the ``8 C + 8`` bytes read and ``8 C``
    bytes written per row; against it the formulation of the same planes with torch ops
    (max, exp, sum, divide, one-hot, the two products, the floor, two casts);
  * ``row_terms``: the fp32 outputs against the NumPy formula in fp64 (``|g - g_np| / max(w, tiny)``,
    ``|h - h_np|``: the fp32 rounding dominates both), what of the first a correct fp32 rounding of the
    NumPy value cannot explain (a witness of the fp64 error; 0 when every element rounds like NumPy's),
    the elements whose fp32 bits differ from NumPy's fp32 rounding, and the elements whose bits
    differ between the host twin and the device;
  * ``fit``: host-clock seconds of a ``--fit-rounds``-round ``fit_gbdt_softprob`` and of a binary ``fit_gbdt``
    of the same rows (``C * --fit-rounds`` rounds, so both grow as many trees), and ms per tree from the
    difference to a fit of ``--fit-short`` rounds, which cancels the quantisation of the features and the
    per-fit set-up (medians of ``--fit-reps`` alternating repetitions; the mean nodes per tree alongside);
  * ``score``: ms of ``score_class_trees`` over ``--score-rounds`` rounds of class trees (the fitted
    rounds repeated) against ``C`` ``score_csr`` calls over the per-class tree lists, and the largest
    difference of the two (their lanes group the trees differently, so they agree to rounding only).

``--md PATH`` also writes the figures as a Markdown profile. ``--dry-run`` walks through every step once
on the host at whatever size is given and measures nothing.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from micro_nb import event_ms, features  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 3, 8])
    ap.add_argument("--fit-rounds", type=int, default=45)
    ap.add_argument("--fit-short", type=int, default=5)
    ap.add_argument("--fit-reps", type=int, default=3)
    ap.add_argument("--score-rounds", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from fraud_detection_spark_kafka_llm_amd.ml.tree_model import class_ensemble_arrays, ensemble_arrays
    from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
    from fraud_detection_spark_kafka_llm_amd.models.gbdt_softprob import fit_gbdt_softprob
    from fraud_detection_spark_kafka_llm_amd.ops import sparse

    dev = torch.device("cpu" if args.dry_run or not torch.cuda.is_available() else "cuda:0")
    reps = 1 if args.dry_run else args.reps
    vc, y2 = features(args.rows, 1, dev)
    N, nnz, F = len(vc), int(vc.csr()[1].numel()), vc.size
    lines = []

    def emit(obj):
        lines.append(obj)
        print(json.dumps(obj), flush=True)

    emit({"data": {"rows": N, "nnz": nnz, "features": F, "device": str(dev)}})
    gen = torch.Generator().manual_seed(5)
    floor = float(sparse.softprob_limits()["min_hess"])

    for C in args.classes:
        # the scam label in the lowest bit, the row number above it: every class has rows of both kinds
        y = ((y2.long() + 2 * (torch.arange(N, device=dev) % ((C + 1) // 2))) % C).to(torch.float32)
        M = (torch.randn((C, N), generator=gen, dtype=torch.float64) * 3.0).to(dev)
        w = torch.tensor([0.3, 0.7, 1.1, 2.9], dtype=torch.float32)[torch.randint(0, 4, (N,), generator=gen)].to(dev)
        G = torch.empty((C, N), dtype=torch.float32, device=dev)
        H = torch.empty((C, N), dtype=torch.float32, device=dev)
        keep = {}

        def parent():
            mx = M.max(dim=0, keepdim=True).values
            e = torch.exp(M - mx)
            p = e / e.sum(dim=0, keepdim=True)
            onehot = (torch.arange(C, device=dev)[:, None] == y.long()[None, :]).to(torch.float64)
            wd = w.to(torch.float64)
            keep["g"] = (wd * (p - onehot)).to(torch.float32)
            keep["h"] = torch.clamp_min(((2.0 * p) * (1.0 - p)) * wd, floor).to(torch.float32)

        ms, lo, hi = event_ms(lambda: sparse.softprob_grad(M, y, w, G, H), reps, torch)
        p_ms, p_lo, p_hi = event_ms(parent, reps, torch)
        moved = (8 * C + 8 + 8 * C) * N
        emit({"grad": {"C": C, "ms": ms, "min": lo, "max": hi, "bytes": moved,
                       "gbytes_per_s": None if ms is None else moved / ms / 1e6,
                       "torch_ms": p_ms, "torch_min": p_lo, "torch_max": p_hi,
                       "torch_over_kernel": None if ms is None else p_ms / ms}})

        # row terms against NumPy fp64
        Mn, yn, wn = M.cpu().numpy(), y.cpu().numpy(), w.cpu().numpy().astype(np.float64)
        mx = Mn.max(axis=0)
        e = np.exp(Mn - mx)
        S = np.zeros_like(mx)
        for c in range(C):
            S = S + e[c]
        p = e / S
        g64 = wn * (p - (np.arange(C)[:, None] == yn[None, :].astype(np.int64)))
        h64 = np.maximum(((2.0 * p) * (1.0 - p)) * wn, floor)
        g, h = G.cpu().numpy(), H.cpu().numpy()
        half = np.spacing(np.abs(g64.astype(np.float32))).astype(np.float64) / 2
        Gh, Hh = torch.empty((C, N), dtype=torch.float32), torch.empty((C, N), dtype=torch.float32)
        sparse.softprob_grad(M.cpu(), y.cpu(), w.cpu(), Gh, Hh)
        emit({"row_terms": {"C": C, "elements": int(g.size),
                            "g_err_per_w": float((np.abs(g - g64) / np.maximum(wn, 1e-300)).max()),
                            "h_err": float(np.abs(h - h64).max()),
                            "g_excess_over_fp32_rounding_per_w": float((np.maximum(np.abs(g - g64) - half, 0) / wn).max()),
                            "g_bits_differ_from_numpy_fp32": int((g != g64.astype(np.float32)).sum()),
                            "h_bits_differ_from_numpy_fp32": int((h != h64.astype(np.float32)).sum()),
                            "g_bits_differ_host_vs_device": int((Gh.numpy() != g).sum()),
                            "h_bits_differ_host_vs_device": int((Hh.numpy() != h).sum())}})

        # the two trainers on the same rows, as many trees each; ms per tree from the difference of a
        # long fit and a short one, so that quantising the features and the per-fit set-up cancel; the
        # four fits alternate --fit-reps times and the medians are taken
        short = 1 if args.dry_run else args.fit_short
        rounds = 2 if args.dry_run else max(args.fit_rounds, short + 1)
        params = dict(max_depth=args.max_depth, max_bin=256)
        yb = y2.to(torch.float32)

        def timed(fn):
            if dev.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if dev.type == "cuda":
                torch.cuda.synchronize()
            return out, time.perf_counter() - t0

        def multi(r):
            return fit_gbdt_softprob(vc, y, GBDTParams(n_estimators=r, **params), device=dev)

        def binary(r):
            return fit_gbdt(vc, yb, GBDTParams(n_estimators=r * C, **params), device=dev)

        multi(1), binary(1)                                                                 # warm-up
        t = {"m1": [], "m2": [], "b1": [], "b2": []}
        for _ in range(1 if args.dry_run else args.fit_reps):
            t["m1"].append(timed(lambda: multi(short))[1])
            res, s2 = timed(lambda: multi(rounds))
            t["m2"].append(s2)
            t["b1"].append(timed(lambda: binary(short))[1])
            bres, s2 = timed(lambda: binary(rounds))
            t["b2"].append(s2)
        med = {k: statistics.median(v) for k, v in t.items()}
        extra = (rounds - short) * C
        nodes = lambda trees: sum(tr.num_nodes for tr in trees) / max(len(trees), 1)      # noqa: E731
        dry = args.dry_run
        emit({"fit": {"C": C, "rounds": rounds, "short_rounds": short, "max_depth": args.max_depth,
                      "trees": len(res.trees), "nodes_per_tree": nodes(res.trees),
                      "seconds": None if dry else med["m2"], "short_seconds": None if dry else med["m1"],
                      "ms_per_tree": None if dry else 1e3 * (med["m2"] - med["m1"]) / extra,
                      "binary_trees": len(bres.trees), "binary_nodes_per_tree": nodes(bres.trees),
                      "binary_seconds": None if dry else med["b2"], "binary_short_seconds": None if dry else med["b1"],
                      "binary_ms_per_tree": None if dry else 1e3 * (med["b2"] - med["b1"]) / extra,
                      "all_seconds": None if dry else t}})

        # scoring: the fitted rounds repeated up to --score-rounds rounds
        want = 1 if args.dry_run else args.score_rounds
        trees = (res.trees * ((want + rounds - 1) // rounds))[: want * C]
        tc = np.arange(len(trees)) % C
        arr = class_ensemble_arrays(trees, tc, C, cmp_less=True)
        per_class = [ensemble_arrays([t for i, t in enumerate(trees) if i % C == c], "value", cmp_less=True)
                     for c in range(C)]

        def grouped():
            keep["raw"] = sparse.score_class_trees(vc, arr)

        def separate():
            keep["cols"] = torch.cat([sparse.score_csr(vc, a) for a in per_class], dim=1)

        s_ms, s_lo, s_hi = event_ms(grouped, reps, torch)
        c_ms, c_lo, c_hi = event_ms(separate, reps, torch)
        emit({"score": {"C": C, "rounds": want, "trees": len(trees), "ms": s_ms, "min": s_lo, "max": s_hi,
                        "score_csr_calls_ms": c_ms, "score_csr_min": c_lo, "score_csr_max": c_hi,
                        "calls_over_grouped": None if s_ms is None else c_ms / s_ms,
                        "max_abs_diff": float((keep["raw"] - keep["cols"]).abs().max())}})

    if args.md:
        write_md(args.md, lines)


def write_md(path, lines):
    by = {}
    for obj in lines:
        for k, v in obj.items():
            by.setdefault(k, []).append(v)
    d = by["data"][0]
    f = lambda v, n=3: "-" if v is None else f"{v:.{n}f}"      # noqa: E731
    out = ["# Multi-class boosting (multi:softprob)", "",
           f"`bench/micro_softprob.py`, one run: {d['rows']} synthetic dialogues, {d['nnz']} stored entries, "
           f"{d['features']} hashed features, device `{d['device']}`. Times are medians by device events "
           "(min .. max in brackets); the fits are host-clock seconds.", "",
           "## softprob_grad", "",
           "| C | kernel ms | GB/s | torch ops ms | torch / kernel |", "|---|---|---|---|---|"]
    for g in by["grad"]:
        out.append(f"| {g['C']} | {f(g['ms'])} [{f(g['min'])} .. {f(g['max'])}] | {f(g['gbytes_per_s'], 1)} | "
                   f"{f(g['torch_ms'])} [{f(g['torch_min'])} .. {f(g['torch_max'])}] | {f(g['torch_over_kernel'], 2)} |")
    out += ["", "## Row terms against the NumPy formula", "",
            "| C | elements | max abs(g - g_np) / w | max abs(h - h_np) | excess over fp32 rounding / w | g bits != NumPy fp32 | "
            "h bits != NumPy fp32 | g host != device | h host != device |", "|---|---|---|---|---|---|---|---|---|"]
    for r in by["row_terms"]:
        out.append(f"| {r['C']} | {r['elements']} | {r['g_err_per_w']:.3e} | {r['h_err']:.3e} | "
                   f"{r['g_excess_over_fp32_rounding_per_w']:.3e} | {r['g_bits_differ_from_numpy_fp32']} | "
                   f"{r['h_bits_differ_from_numpy_fp32']} | {r['g_bits_differ_host_vs_device']} | "
                   f"{r['h_bits_differ_host_vs_device']} |")
    out += ["", "## Fits", "",
            "| C | rounds (short) | trees | nodes / tree | multi:softprob s (short s) | ms / tree | binary nodes / tree | "
            "binary s (short s) | binary ms / tree |", "|---|---|---|---|---|---|---|---|---|"]
    for r in by["fit"]:
        out.append(f"| {r['C']} | {r['rounds']} ({r['short_rounds']}) | {r['trees']} | {f(r['nodes_per_tree'], 1)} | "
                   f"{f(r['seconds'])} ({f(r['short_seconds'])}) | {f(r['ms_per_tree'], 2)} | "
                   f"{f(r['binary_nodes_per_tree'], 1)} | {f(r['binary_seconds'])} ({f(r['binary_short_seconds'])}) | "
                   f"{f(r['binary_ms_per_tree'], 2)} |")
    out += ["", "## score_class_trees", "",
            "| C | rounds | trees | grouped ms | C score_csr calls ms | calls / grouped | max abs difference |",
            "|---|---|---|---|---|---|---|"]
    for r in by["score"]:
        out.append(f"| {r['C']} | {r['rounds']} | {r['trees']} | {f(r['ms'])} [{f(r['min'])} .. {f(r['max'])}] | "
                   f"{f(r['score_csr_calls_ms'])} [{f(r['score_csr_min'])} .. {f(r['score_csr_max'])}] | "
                   f"{f(r['calls_over_grouped'], 2)} | {r['max_abs_diff']:.3e} |")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
