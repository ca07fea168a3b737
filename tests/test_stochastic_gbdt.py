"""Row and column subsampling of the GBDT trainer (``GBDTParams.subsample`` / ``colsample_by*``,
``SparkXGBClassifier(subsample=..., colsample_bytree=...)``).

Contract (README "Stochastic boosting"): round ``t`` keeps the row with global index ``i`` iff
``hash_uniform(seed, t, i) < subsample``; a row that is not kept has g = h = 0 for that tree, is
still partitioned and still receives the tree's leaf value; the quantisation exponents stay the
round's max |g|, |h| over every row. The oracle is ``rf_sampling.row_keep_mask`` plus a NumPy
exact-histogram Newton booster written here (the one of tests/test_oracles.py with the mask).
Columns: nested stages of exactly k features (tree, level, node) by k-th smallest counter-based
priority; the oracle is ``rf_sampling.column_thresholds``."""
import json
import math

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.base import Params
from fraud_detection_spark_kafka_llm_amd.ml.frame import Frame
from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import ensemble_arrays
from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier, SparkXGBClassifierModel
from fraud_detection_spark_kafka_llm_amd.models import rf_sampling
from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
from fraud_detection_spark_kafka_llm_amd.ops import native
from fraud_detection_spark_kafka_llm_amd.ops.sparse import score_csr
from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
N_ROWS, SEED = 6000, 5
KW = dict(n_estimators=4, max_depth=3, learning_rate=0.3, reg_lambda=1.0, gamma=0.5, min_child_weight=2.0,
          max_bin=64, seed=SEED)


def _int_features(n: int, seed: int) -> tuple:
    """Integer features with 9..24 distinct values each (zero included, some negative, so the zero
    bin sits inside the range) and a noisy non-linear label: 64 bins are lossless."""
    rng = np.random.default_rng(seed)
    F = 10
    X = np.zeros((n, F))
    for f in range(F):
        vals = rng.integers(-(f % 4), 8 + 2 * f if f < 8 else 12, n)
        X[:, f] = np.where(rng.random(n) < (0.55 + 0.04 * f), vals, 0)
    score = (1.3 * (X[:, 0] > 3) + 0.9 * (X[:, 2] * X[:, 5] > 20) - 0.8 * (X[:, 7] < 2) + 0.05 * X[:, 9]
             + 0.4 * np.sin(X[:, 4]))
    y = (score + rng.normal(0, 0.6, n) > 0.6).astype(np.float32)
    return X, y


def _csr_vc(X: np.ndarray) -> VectorColumn:
    nz = X != 0
    indptr = np.zeros(X.shape[0] + 1, dtype=np.int64)
    np.cumsum(nz.sum(1), out=indptr[1:])
    r, c = np.nonzero(nz)
    return VectorColumn(X.shape[1], torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int32)),
                        torch.from_numpy(X[r, c].astype(np.float64)))


def _sig(trees):
    return [(t.feature.tolist(), t.threshold.tolist(), t.stats.tolist()) for t in trees]


_DATA: dict = {}


def _data():
    if not _DATA:
        X, y = _int_features(N_ROWS, 11)
        _DATA.update(X=X, y=y, vc=_csr_vc(X), yt=torch.from_numpy(y))
    return _DATA


_FITS: dict = {}


def _host_fit(**over):
    """Host fits shared by the tests (computed once per parameter set, never changed)."""
    key = tuple(sorted(over.items()))
    if key not in _FITS:
        d = _data()
        _FITS[key] = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **over}), device="cpu")
    return _FITS[key]


# ------------------------------------------------------------------------------- 1. the row mask
def _undigits4(d: np.ndarray) -> np.ndarray:
    return (d.astype(np.uint32) ^ np.uint32(0x80808080)).astype(np.int64) - 0x80808080


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("subsample", [0.5, 0.1])
def test_quantisation_zeroes_exactly_the_rows_the_oracle_drops(device, subsample):
    """Sizes: the wave (64), the 1024 rows a workgroup takes per step, their neighbours and tails."""
    C = native.lib()
    rng = np.random.default_rng(3)
    # (... and a size the host twin splits among its threads at boundaries that are no multiple of 64)
    for N in (1, 63, 64, 65, 1023, 1024, 1025, 4097, 3 * 65536 + 17):
        g = torch.from_numpy(rng.normal(0, 0.3, N).astype(np.float32)).to(device)
        h = torch.from_numpy(rng.uniform(0.01, 0.25, N).astype(np.float32)).to(device)
        mx = torch.zeros(2, dtype=torch.float64, device=device)
        C.tree_quant_max(g, h, None, None, SEED, 0, False, 0, N, mx, 0)
        assert mx.tolist() == [float(g.abs().max()), float(h.abs().max())]

        def quant(rnd, row0, ss):
            dig = torch.full((N, 2), -1, dtype=torch.int32, device=device)
            kexp = torch.zeros(2, dtype=torch.int32, device=device)
            tot = torch.zeros(2, dtype=torch.int64, device=device)
            bits = torch.full(((N + 63) // 64,), -1, dtype=torch.int64, device=device)
            C.tree_quant(g, h, None, None, SEED, rnd, False, 0, 4, mx, dig, kexp, tot, None, row0, ss, bits)
            if ss < 1.0:            # one keep bit per row (bit r & 63 of word r >> 6), zero past the end
                got = (bits.cpu().numpy().view(np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
                want = np.zeros(bits.numel() * 64, dtype=np.uint64)
                want[:N] = rf_sampling.row_keep_mask(SEED, rnd, row0, N, ss).numpy()
                assert np.array_equal(got.reshape(-1), want), (N, rnd, row0)
            return dig.cpu().numpy(), kexp.tolist(), tot.tolist()

        full, kfull, _ = quant(0, 0, 1.0)
        for rnd in (0, 99):
            for row0 in (0, 12345):
                keep = rf_sampling.row_keep_mask(SEED, rnd, row0, N, subsample).numpy()
                dig, kexp, tot = quant(rnd, row0, subsample)
                assert kexp == kfull                    # the exponents cover every row, kept or not
                assert not dig[~keep].any()
                assert np.array_equal(dig[keep], full[keep])
                q = _undigits4(full)
                assert tot == [int(q[keep, 0].sum()), int(q[keep, 1].sum())], (N, rnd, row0)


def test_kept_fraction_is_within_five_sigma():
    N = 20000
    for p in (0.5, 0.1, 0.9):
        bound = 5.0 * math.sqrt(p * (1 - p) / N)
        for seed in (0, 7, 42):
            for rnd in (0, 1, 99):
                for row0 in (0, 12345):
                    kept = int(rf_sampling.row_keep_mask(seed, rnd, row0, N, p).sum())
                    assert abs(kept / N - p) <= bound, (p, seed, rnd, row0, kept)
    # different rounds and different shards of the same round draw different rows
    a, b = rf_sampling.row_keep_mask(0, 0, 0, N, 0.5), rf_sampling.row_keep_mask(0, 1, 0, N, 0.5)
    assert 0.4 < float((a != b).float().mean()) < 0.6
    assert torch.equal(rf_sampling.row_keep_mask(0, 0, 0, N, 0.5)[100:],
                       rf_sampling.row_keep_mask(0, 0, 100, N - 100, 0.5))
    assert bool(rf_sampling.row_keep_mask(0, 0, 0, 10, 1.0).all())


# ------------------------------------------------------------------------------- 2. the row lists
def _pack_bits(keep: np.ndarray) -> torch.Tensor:
    pad = np.zeros((len(keep) + 63) // 64 * 64, dtype=np.uint8)
    pad[:len(keep)] = keep
    return torch.from_numpy(np.packbits(pad, bitorder="little").view(np.int64).copy())


def _list_case(dev, n, ns, subsample, rnd=3, row0=12345, counted=False):
    """The rows of each slot that round ``rnd`` keeps (handed over as the quantisation's keep bits),
    ascending: (slot starts, list, digit words)."""
    C = native.lib()
    rng = np.random.default_rng(n + ns)
    row_node = rng.integers(-1, 2 * ns + 2, n).astype(np.int32)
    node_slot = np.full(2 * ns + 1, -1, dtype=np.int32)
    node_slot[rng.permutation(2 * ns + 1)[:ns]] = np.arange(ns, dtype=np.int32)
    sl = np.where((row_node >= 0) & (row_node < node_slot.size), node_slot[np.clip(row_node, 0, node_slot.size - 1)], -1)
    keep = rf_sampling.row_keep_mask(SEED, rnd, row0, n, subsample).numpy()
    lst = torch.full((n,), -7, dtype=torch.int32, device=dev)
    start = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    # (stale counts of every row, as the partition leaves them: the subsampled list counts its own)
    work = torch.full((ns * (2 + n // C.tree_rg_list_rows(n) + 1),), 99, dtype=torch.int32, device=dev)
    dig = torch.from_numpy(rng.integers(0, 1 << 30, (n, 2)).astype(np.int32)).to(dev)
    ldig = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    masked = torch.full((n, 2), -1, dtype=torch.int32, device=dev) if ns == 1 else None
    C.tree_rg_list(torch.from_numpy(row_node).to(dev), torch.from_numpy(node_slot).to(dev), None, n, ns, work, start,
                   lst, dig, ldig, masked, counted=counted, keepbits=_pack_bits(keep).to(dev) if subsample < 1.0 else None)
    st, lst, ldig = start.cpu().numpy(), lst.cpu().numpy(), ldig.cpu().numpy()
    for s in range(ns):
        np.testing.assert_array_equal(lst[st[s]:st[s + 1]], np.nonzero((sl == s) & keep)[0])
    assert st[0] == 0 and st[-1] == ((sl >= 0) & keep).sum() and (lst[st[-1]:] == -7).all()
    np.testing.assert_array_equal(ldig[:st[-1]], dig.cpu().numpy()[lst[:st[-1]]])
    if masked is not None:       # every row's digit words, zero outside the kept rows of slot 0
        want = np.where(((sl == 0) & keep)[:, None], dig.cpu().numpy(), 0)
        np.testing.assert_array_equal(masked.cpu().numpy(), want)
    return st, lst[:st[-1]]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("ns", [1, 2, 5])
def test_row_lists_hold_the_kept_rows_of_each_slot(device, ns):
    """512-row list waves: one wave short, exact, one over, and several blocks."""
    for n in (511, 512, 513, 2049):
        for p in (0.5, 0.1):
            got = _list_case(device, n, ns, p, counted=(n == 2049))
            if device != "cpu":
                want = _list_case("cpu", n, ns, p)
                assert all(np.array_equal(a, b) for a, b in zip(got, want))
    full = _list_case(device, 2049, ns, 1.0)             # (subsample 1: every row of the built nodes)
    assert len(full[1]) > len(_list_case(device, 2049, ns, 0.5)[1])


@pytest.mark.parametrize("device", DEVICES)
def test_row_lists_with_2048_row_waves(device):
    C = native.lib()
    old = C.tree_set_list_big_rows(1000)
    try:
        assert C.tree_rg_list_rows(5000) == 2048
        for ns in (1, 5):
            _list_case(device, 5000, ns, 0.5)
    finally:
        C.tree_set_list_big_rows(old)


# ------------------------------------------------------------------------------- 4. trees against an oracle
def _quant_exponent(m: float) -> int:
    return 30 - math.frexp(m)[1] if m > 0 else 0


def _oracle_tree(Xb, nbins, g, h, keep, params, eligible=None, used=None):
    """One depth-wise tree on exact integer sums over the kept rows (exponents from every row);
    returns the leaf value of every row, kept or not, and the list of leaf values."""
    k0 = _quant_exponent(float(np.abs(g.astype(np.float64)).max()))
    k1 = _quant_exponent(float(np.abs(h.astype(np.float64)).max()))
    q0 = np.where(keep, np.rint(np.ldexp(g.astype(np.float64), k0)), 0).astype(np.int64)
    q1 = np.where(keep, np.rint(np.ldexp(h.astype(np.float64), k1)), 0).astype(np.int64)
    s0, s1 = math.ldexp(1.0, -k0), math.ldexp(1.0, -k1)
    lam, mcw = params.reg_lambda, params.min_child_weight
    n, F = Xb.shape
    node_of = np.zeros(n, dtype=np.int64)
    leaf_value = np.zeros(n)
    nodes, next_id, leaves = [(0, 0)], 1, []
    while nodes:
        nid, d = nodes.pop(0)
        rows = np.nonzero(node_of == nid)[0]
        T0, T1 = int(q0[rows].sum()), int(q1[rows].sum())
        G, H = T0 * s0, T1 * s1
        best = None
        if d < params.max_depth:
            parent = G * G / (H + lam)
            ok = eligible(d, nid) if eligible is not None else np.ones(F, dtype=bool)
            for f in range(F):
                if not ok[f]:
                    continue
                a0 = np.zeros(nbins[f], dtype=np.int64)
                a1 = np.zeros(nbins[f], dtype=np.int64)
                np.add.at(a0, Xb[rows, f], q0[rows])
                np.add.at(a1, Xb[rows, f], q1[rows])
                l0 = l1 = 0
                for b in range(nbins[f] - 1):
                    l0 += int(a0[b])
                    l1 += int(a1[b])
                    L1, R1 = l1 * s1, (T1 - l1) * s1
                    if L1 < mcw or R1 < mcw:
                        continue
                    L0, R0 = l0 * s0, (T0 - l0) * s0
                    gain = L0 * L0 / (L1 + lam) + R0 * R0 / (R1 + lam) - parent
                    if best is None or gain > best[0]:
                        best = (gain, f, b)
        if best is not None and best[0] > max(params.gamma, 1e-6):
            _, f, b = best
            if used is not None:
                used.append((nid, d, f))
            node_of[rows[Xb[rows, f] <= b]] = next_id
            node_of[rows[Xb[rows, f] > b]] = next_id + 1
            nodes += [(next_id, d + 1), (next_id + 1, d + 1)]
            next_id += 2
            continue
        v = params.learning_rate * (-G / (H + lam))
        leaf_value[rows] = v
        leaves.append(v)
    return leaf_value, leaves


@pytest.mark.parametrize("device", DEVICES)
def test_subsampled_trees_equal_numpy_exact_histogram_oracle(device):
    """Leaf values and the margins of all rows, to the 1e-12 of the unsampled oracle test."""
    d = _data()
    X, y = d["X"], d["y"]
    vals = [np.unique(X[:, f]) for f in range(X.shape[1])]
    Xb = np.stack([np.searchsorted(vals[f], X[:, f]) for f in range(X.shape[1])], 1)
    params = GBDTParams(**{**KW, "subsample": 0.5})
    margins = []
    ours = fit_gbdt(d["vc"], d["yt"], params, device=device,
                    eval_fn=lambda t, trees, m: margins.append(m.detach().cpu().numpy().copy()))
    assert len(ours.trees) == params.n_estimators
    ybar = float(y.astype(np.float64).mean())
    margin = np.full(len(y), math.log(ybar / (1 - ybar)))
    assert ours.base_margin == pytest.approx(margin[0], abs=1e-12)      # (every row, not the kept ones)
    for t, tree in enumerate(ours.trees):
        p = 1.0 / (1.0 + np.exp(-margin))
        g = (p - y.astype(np.float64)).astype(np.float32)
        h = np.maximum(p * (1.0 - p), 1e-16).astype(np.float32)
        keep = rf_sampling.row_keep_mask(SEED, t, 0, len(y), 0.5).numpy()
        ov, leaves = _oracle_tree(Xb, [len(v) for v in vals], g, h, keep, params)
        got = score_csr(d["vc"], ensemble_arrays([tree], "value", cmp_less=False))[:, 0].numpy()
        np.testing.assert_allclose(got, ov, rtol=0, atol=1e-12, err_msg=f"tree {t}")
        ours_leaves = sorted(float(tree.stats[i, 0]) for i in range(tree.num_nodes) if tree.feature[i] < 0)
        np.testing.assert_allclose(ours_leaves, sorted(leaves), rtol=0, atol=1e-12)
        # the root's cover is the hessian sum of the kept rows alone
        assert float(tree.stats[tree.root, 1]) == pytest.approx(float(h[keep].astype(np.float64).sum()), rel=1e-6)
        margin = margin + ov
        # ... and the trainer's own margins moved on every row, kept or not
        np.testing.assert_allclose(margins[t], margin, rtol=0, atol=1e-11)
    assert _sig(ours.trees) != _sig(_host_fit().trees)


def test_host_level_loop_equals_device_level_loop_on_the_host(monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.models import grower

    want = _host_fit(subsample=0.5)
    monkeypatch.setattr(grower, "DEVICE_LEVELS", False)
    d = _data()
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, "subsample": 0.5}), device="cpu")
    assert _sig(got.trees) == _sig(want.trees)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [None, "ROWHIST", "DEVICE_LEVELS", "NATIVE_LEVELS", "GBDT_CXX_LEVELS"])
@pytest.mark.parametrize("subsample", [0.5, 0.8])
def test_every_device_loop_grows_the_host_trees(flip, subsample, monkeypatch):
    """C++ runner (default) = CSC passes = host level loop = Python device loop = generic runner
    levels, bitwise the host fit."""
    from fraud_detection_spark_kafka_llm_amd.models import grower

    if flip is not None:
        monkeypatch.setattr(grower, flip, False)
    d = _data()
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, "subsample": subsample}), device="cuda:0")
    assert _sig(got.trees) == _sig(_host_fit(subsample=subsample).trees)


@pytest.mark.gpu
def test_depth_six_device_equals_host():
    """Sibling subtraction and multi-slot row lists over rows whose digit words are zero."""
    d = _data()
    over = dict(max_depth=6, gamma=0.0, min_child_weight=1.0, subsample=0.5)
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **over}), device="cuda:0")
    want = _host_fit(**over)
    assert _sig(got.trees) == _sig(want.trees)
    assert max(t.num_nodes for t in want.trees) > 31           # (deeper than 4 levels)


@pytest.mark.gpu
def test_large_shard_list_waves_equal_host():
    """2048-row list waves: the partition keeps rows per node (not the lists' counts), which the
    subsampled lists must not use either."""
    C = native.lib()
    old = C.tree_set_list_big_rows(1000)
    try:
        assert not C.tree_partition_counts_ok(N_ROWS)
        d = _data()
        over = dict(max_depth=5, gamma=0.0, min_child_weight=1.0, subsample=0.5)
        got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **over}), device="cuda:0")
    finally:
        C.tree_set_list_big_rows(old)
    assert _sig(got.trees) == _sig(_host_fit(**over).trees)


# ------------------------------------------------------------------------------- 3. column thresholds
def _native_thresholds(dev, F, tree, depth, nodes, fractions):
    """(thr_tree, thr_level, thr_node) through the kernels (device) or their host twins (cpu), queued
    as the trainer queues them (grower.ColumnSampler)."""
    from types import SimpleNamespace

    from fraud_detection_spark_kafka_llm_amd.models import grower

    Q = SimpleNamespace(device=torch.device(dev), num_features=F)
    params = SimpleNamespace(max_depth=depth + 1, colsample_bytree=fractions[0], colsample_bylevel=fractions[1],
                             colsample_bynode=fractions[2])
    col = grower.ColumnSampler(Q, params, (tuple(fractions), depth + 1))
    C = native.lib()
    col.begin(C, SEED, tree)
    ids = torch.tensor(nodes, dtype=torch.int32, device=dev)
    thr, kw = col.level_args(C, SEED, tree, depth, ids)
    thr = torch.ones(len(nodes), dtype=torch.float64) if thr is None else thr.cpu()
    mask = kw["col_mask"].cpu().bool() if kw.get("col_mask") is not None else None
    return float(col.tree[0]), float(col.level[depth]), thr, col.ks, mask


# kCap = 2048 candidates are ranked in LDS (rf_kernels.hip): at most that many features skip the
# radix passes; 2049 and 2^18 take them
COL_F = [1, 2, 63, 64, 65, 1000, 2048, 2049, 1 << 18]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", COL_F)
def test_column_thresholds_equal_the_oracle(device, F):
    near_one = lambda n: (n - 0.5) / n                 # noqa: E731  (keeps n - 1 of n)
    k1 = 0.5 / F                                         # (keeps max(1, 0) = 1)
    cases = [(0.5, 0.5, 0.5), (k1, 1.0, 1.0), (1.0, k1, 1.0), (1.0, 1.0, k1), (0.5, 1.0, 0.5),
             (near_one(F), 1.0, 1.0), (0.5, near_one(max(1, int(0.5 * F))), 1.0), (1.0, 0.5, near_one(max(1, int(0.5 * F))))]
    nodes, tree, depth = [3, 4, 9], 7, 2
    for fr in cases:
        t_tree, t_level, t_node, elig = rf_sampling.column_thresholds(F, SEED, tree, depth, nodes, *fr)
        g_tree, g_level, g_node, ks, g_mask = _native_thresholds(device, F, tree, depth, nodes, fr)
        assert (g_tree, g_level) == (t_tree, t_level), (F, fr)
        assert torch.equal(g_node, t_node), (F, fr)
        # exactly k features pass each stage, and the stages are nested
        fid = torch.arange(F, dtype=torch.int64)
        p_tree = rf_sampling._priorities(SEED, tree, rf_sampling.COL_TREE_KEY, fid) <= t_tree
        p_level = p_tree & (rf_sampling._priorities(SEED, tree, rf_sampling.COL_LEVEL_KEY - depth, fid) <= t_level)
        if g_mask is not None:                      # the level's byte mask = the two outer stages
            assert torch.equal(g_mask, p_level), (F, fr)
        n = F
        for k, passing in zip(ks[:2], (p_tree, p_level)):
            n = k or n
            assert int(passing.sum()) == n, (F, fr)
        for i in range(len(nodes)):
            assert int(elig[i].sum()) == (ks[2] or n) and bool((elig[i] <= p_level).all()), (F, fr, i)
    assert rf_sampling.column_counts(F, 1.0, 1.0, 1.0) == (0, 0, 0)


def test_priorities_of_one_key_are_distinct():
    fid = torch.arange(1 << 18, dtype=torch.int64)
    for key in (rf_sampling.COL_TREE_KEY, rf_sampling.COL_LEVEL_KEY - 3, 5):
        assert torch.unique(rf_sampling._priorities(SEED, 2, key, fid)).numel() == 1 << 18


@pytest.mark.parametrize("device", DEVICES)
def test_unfiltered_rf_sample_is_unchanged(device):
    C = native.lib()
    F, k, nodes = 5000, 71, [0, 5, 6, -1]
    fid = torch.arange(0, F, 3, dtype=torch.int64, device=device)
    thr = torch.zeros(len(nodes), dtype=torch.float64, device=device)
    mask = torch.zeros(fid.numel(), dtype=torch.uint8, device=device)
    C.tree_rf_sample(SEED, 4, torch.tensor(nodes, dtype=torch.int32, device=device), F, k, fid, thr, mask, None)
    want = rf_sampling.node_thresholds(F, SEED, 4, nodes[:3], k, "cpu")
    assert torch.equal(thr.cpu()[:3], want) and float(thr[3]) == -1.0


# ------------------------------------------------------------------------------- 4b. column-sampled trees
COL_CASES = {"columns": dict(colsample_bytree=0.5, colsample_bylevel=0.5, colsample_bynode=0.5),
             "bytree": dict(colsample_bytree=0.5), "bynode": dict(colsample_bynode=0.5),
             "rows+columns": dict(subsample=0.5, colsample_bytree=0.5, colsample_bylevel=0.5, colsample_bynode=0.5)}


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("case", ["columns", "rows+columns"])
def test_column_sampled_trees_equal_numpy_exact_histogram_oracle(device, case):
    d = _data()
    X, y = d["X"], d["y"]
    F = X.shape[1]
    over = COL_CASES[case]
    fr = (over["colsample_bytree"], over["colsample_bylevel"], over["colsample_bynode"])
    vals = [np.unique(X[:, f]) for f in range(F)]
    Xb = np.stack([np.searchsorted(vals[f], X[:, f]) for f in range(F)], 1)
    params = GBDTParams(**{**KW, **over})
    ours = fit_gbdt(d["vc"], d["yt"], params, device=device)
    ybar = float(y.astype(np.float64).mean())
    margin = np.full(len(y), math.log(ybar / (1 - ybar)))
    for t, tree in enumerate(ours.trees):
        p = 1.0 / (1.0 + np.exp(-margin))
        g = (p - y.astype(np.float64)).astype(np.float32)
        h = np.maximum(p * (1.0 - p), 1e-16).astype(np.float32)
        keep = rf_sampling.row_keep_mask(SEED, t, 0, len(y), over.get("subsample", 1.0)).numpy()
        used = []
        elig = lambda depth, nid: rf_sampling.column_thresholds(F, SEED, t, depth, [nid], *fr)[3][0].numpy()  # noqa: E731
        ov, leaves = _oracle_tree(Xb, [len(v) for v in vals], g, h, keep, params, elig, used)
        got = score_csr(d["vc"], ensemble_arrays([tree], "value", cmp_less=False))[:, 0].numpy()
        np.testing.assert_allclose(got, ov, rtol=0, atol=1e-12, err_msg=f"tree {t}")
        ours_leaves = sorted(float(tree.stats[i, 0]) for i in range(tree.num_nodes) if tree.feature[i] < 0)
        np.testing.assert_allclose(ours_leaves, sorted(leaves), rtol=0, atol=1e-12)
        # every internal node's feature is eligible for that node, and the oracle chose the same ones
        assert sorted(f for _, _, f in used) == sorted(int(f) for f in tree.feature if f >= 0)
        assert all(elig(depth, nid)[f] for nid, depth, f in used)
        margin = margin + ov
    assert _sig(ours.trees) != _sig(_host_fit(**{k: v for k, v in over.items() if k == "subsample"}).trees)


@pytest.mark.parametrize("case", sorted(COL_CASES))
def test_column_sampling_host_level_loop_equals_device_level_loop_on_the_host(case, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.models import grower

    want = _host_fit(**COL_CASES[case])
    monkeypatch.setattr(grower, "DEVICE_LEVELS", False)
    d = _data()
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **COL_CASES[case]}), device="cpu")
    assert _sig(got.trees) == _sig(want.trees)


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [None, "ROWHIST", "DEVICE_LEVELS", "NATIVE_LEVELS", "GBDT_CXX_LEVELS"])
@pytest.mark.parametrize("case", sorted(COL_CASES))
def test_column_sampling_every_device_loop_grows_the_host_trees(flip, case, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.models import grower

    if flip is not None:
        monkeypatch.setattr(grower, flip, False)
    d = _data()
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **COL_CASES[case]}), device="cuda:0")
    assert _sig(got.trees) == _sig(_host_fit(**COL_CASES[case]).trees)


@pytest.mark.gpu
def test_column_sampling_depth_six_device_equals_host():
    """Sibling subtraction inside the split search must not depend on the sampled features: a
    feature masked at one level is a parent row of the next."""
    d = _data()
    over = dict(max_depth=6, gamma=0.0, min_child_weight=1.0, **COL_CASES["rows+columns"])
    got = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **over}), device="cuda:0")
    want = _host_fit(**over)
    assert _sig(got.trees) == _sig(want.trees)
    assert max(t.num_nodes for t in want.trees) > 15


def _rank_fit_cols(rank, world, device="cpu"):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = _int_features(N_ROWS, 11)
    lo, hi = shard_range(N_ROWS, rank, world)
    res = fit_gbdt(_csr_vc(X[lo:hi]), torch.from_numpy(y[lo:hi]),
                   GBDTParams(**{**KW, **COL_CASES["rows+columns"]}), device=device)
    return _sig(res.trees)


def test_column_sampling_resume_num_workers_and_early_stopping(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.parallel.checkpoint import InjectedFault

    d = _data()
    p = GBDTParams(**{**KW, **COL_CASES["rows+columns"], "n_estimators": 8})
    ref = fit_gbdt(d["vc"], d["yt"], p, device="cpu")
    ck = dict(checkpoint_dir=str(tmp_path / "ck"), checkpoint_every=2)
    monkeypatch.setenv("FDX_FAULT", "tree:5")
    with pytest.raises(InjectedFault):
        fit_gbdt(d["vc"], d["yt"], p, device="cpu", **ck)
    monkeypatch.delenv("FDX_FAULT")
    assert _sig(fit_gbdt(d["vc"], d["yt"], p, device="cpu", resume=True, **ck).trees) == _sig(ref.trees)
    # early stopping keeps a prefix of the plain column-sampled fit
    tr, ytr, va, yva = _csr_vc(d["X"][:4000]), d["yt"][:4000], _csr_vc(d["X"][4000:]), d["yt"][4000:]
    p40 = GBDTParams(**{**KW, **COL_CASES["rows+columns"], "n_estimators": 40, "max_depth": 4, "gamma": 0.0})
    plain = fit_gbdt(tr, ytr, p40, device="cpu")
    es = fit_gbdt(tr, ytr, p40, device="cpu", eval_set=(va, yva, None), eval_metric="logloss", early_stopping_rounds=3)
    assert 0 < len(es.trees) == es.best_iteration + 1 < 40 and _sig(es.trees) == _sig(plain.trees[:len(es.trees)])
    # num_workers = 2 through the estimator
    monkeypatch.setenv("FDX_DP_MIN_ROWS", "0")
    kw = dict(COL_CASES["rows+columns"], **EST_KW)
    single = SparkXGBClassifier(**kw).fit(_frame())
    multi = SparkXGBClassifier(num_workers=2, **kw).fit(_frame())
    assert _sig(multi.trees) == _sig(single.trees)


def test_column_sampling_data_parallel_trees_are_bitwise_world_one():
    single = _sig(_host_fit(**COL_CASES["rows+columns"]).trees)
    for world in (2, 3):
        outs = spawn(_rank_fit_cols, world, backend="gloo", timeout=300)
        assert all(o == single for o in outs), world


@pytest.mark.gpu
def test_column_sampling_forced_collectives_on_the_gpu_equal_the_host_fit(monkeypatch):
    monkeypatch.setenv("FDX_FORCE_COLLECTIVES", "1")
    got, = spawn(_rank_fit_cols, 1, "cuda:0", backend="nccl", timeout=300)
    assert got == _sig(_host_fit(**COL_CASES["rows+columns"]).trees)


# ------------------------------------------------------------------------------- 5. invariants
def _frame(n=N_ROWS):
    d = _data()
    return Frame({"features": _csr_vc(d["X"][:n]), "label": d["y"][:n].astype(np.float64)})


EST_KW = dict(features_col="features", label_col="label", n_estimators=4, max_depth=3, seed=SEED)


@pytest.mark.parametrize("device", DEVICES)
def test_explicit_one_equals_the_default(device):
    d = _data()
    a = fit_gbdt(d["vc"], d["yt"], GBDTParams(**KW), device=device)
    ones = dict(subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, colsample_bynode=1.0)
    b = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, **ones}), device=device)
    assert _sig(a.trees) == _sig(b.trees) == _sig(_host_fit().trees)


def test_explicit_one_saves_the_same_model_bytes(tmp_path):
    a = SparkXGBClassifier(uid="x", **EST_KW).fit(_frame())
    b = SparkXGBClassifier(uid="x", subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, colsample_bynode=1.0,
                           **EST_KW).fit(_frame())
    a.save(tmp_path / "a")
    b.save(tmp_path / "b")
    assert (tmp_path / "a" / "model" / "part-00000").read_bytes() == (tmp_path / "b" / "model" / "part-00000").read_bytes()


def test_margins_are_base_plus_each_tree_on_every_row():
    d = _data()
    last = {}
    res = fit_gbdt(d["vc"], d["yt"], GBDTParams(**{**KW, "subsample": 0.5}), device="cpu",
                   eval_fn=lambda t, trees, m: last.update(m=m.clone()))
    m = torch.full((N_ROWS,), res.base_margin, dtype=torch.float64)
    for tr in res.trees:
        m += score_csr(d["vc"], ensemble_arrays([tr], "value", cmp_less=False))[:, 0]
    assert torch.equal(last["m"], m)


def test_treeshap_rows_sum_to_the_raw_prediction():
    model = SparkXGBClassifier(subsample=0.5, **EST_KW).fit(_frame())
    vc = _data()["vc"]
    paths = model.paths()
    raw1 = model.postprocess(score_csr(vc, model.scorer()))[0][:, 1]
    ptr, idx, val = model.contributions(vc).csr()
    tol = 1e-10 * (float(np.abs(paths.path_v).sum()) + abs(model.base_margin))
    assert float((val.view(len(vc), -1).sum(1) - raw1).abs().max()) <= tol


def test_early_stopping_keeps_a_prefix_of_the_subsampled_fit():
    d = _data()
    n_tr = 4000
    tr, ytr = _csr_vc(d["X"][:n_tr]), d["yt"][:n_tr]
    va, yva = _csr_vc(d["X"][n_tr:]), d["yt"][n_tr:]
    p = GBDTParams(**{**KW, "n_estimators": 40, "max_depth": 4, "gamma": 0.0, "subsample": 0.5})
    plain = fit_gbdt(tr, ytr, p, device="cpu")
    es = fit_gbdt(tr, ytr, p, device="cpu", eval_set=(va, yva, None), eval_metric="logloss", early_stopping_rounds=3)
    assert 0 < len(es.trees) == es.best_iteration + 1 < 40
    assert _sig(es.trees) == _sig(plain.trees[:len(es.trees)])


# ------------------------------------------------------------------------------- 6. distribution and restart
def _rank_fit(rank, world, device="cpu", ck=None, resume=False, subsample=0.5, n_estimators=4):
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    X, y = _int_features(N_ROWS, 11)
    lo, hi = shard_range(N_ROWS, rank, world)
    kw = dict(checkpoint_dir=ck, checkpoint_every=2, resume=resume) if ck else {}
    res = fit_gbdt(_csr_vc(X[lo:hi]), torch.from_numpy(y[lo:hi]),
                   GBDTParams(**{**KW, "subsample": subsample, "n_estimators": n_estimators}), device=device, **kw)
    return _sig(res.trees)


def test_data_parallel_trees_are_bitwise_world_one():
    single = _sig(_host_fit(subsample=0.5).trees)
    for world in (2, 3):
        outs = spawn(_rank_fit, world, backend="gloo", timeout=300)
        assert all(o == single for o in outs), world


@pytest.mark.gpu
def test_forced_collectives_on_the_gpu_equal_the_host_fit(monkeypatch):
    monkeypatch.setenv("FDX_FORCE_COLLECTIVES", "1")
    got, = spawn(_rank_fit, 1, "cuda:0", backend="nccl", timeout=300)
    assert got == _sig(_host_fit(subsample=0.5).trees)


def test_num_workers_equals_single_process(monkeypatch):
    monkeypatch.setenv("FDX_DP_MIN_ROWS", "0")
    single = SparkXGBClassifier(subsample=0.5, **EST_KW).fit(_frame())
    multi = SparkXGBClassifier(subsample=0.5, num_workers=2, **EST_KW).fit(_frame())
    assert _sig(multi.trees) == _sig(single.trees)
    assert _sig(single.trees) != _sig(SparkXGBClassifier(**EST_KW).fit(_frame()).trees)


def test_resume_equals_the_uninterrupted_fit(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.parallel.checkpoint import EnsembleCheckpointer, InjectedFault

    ref = _rank_fit(0, 1, n_estimators=8)
    ck = str(tmp_path / "ck")
    monkeypatch.setenv("FDX_FAULT", "tree:5")
    with pytest.raises(InjectedFault):
        _rank_fit(0, 1, ck=ck, n_estimators=8)
    monkeypatch.delenv("FDX_FAULT")
    st = EnsembleCheckpointer(ck).load()
    assert st["trees_done"] == 6 and st["params"]["subsample"] == 0.5
    assert _rank_fit(0, 1, ck=ck, resume=True, n_estimators=8) == ref
    # another fraction is another run
    with pytest.raises(RuntimeError, match="different parameters"):
        _rank_fit(0, 1, ck=ck, resume=True, subsample=0.8, n_estimators=8)


def test_checkpoint_written_before_the_parameter_existed_resumes(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.parallel.checkpoint import EnsembleCheckpointer, InjectedFault

    ref = _rank_fit(0, 1, subsample=1.0, n_estimators=8)
    ck = str(tmp_path / "ck")
    monkeypatch.setenv("FDX_FAULT", "tree:5")
    with pytest.raises(InjectedFault):
        _rank_fit(0, 1, ck=ck, subsample=1.0, n_estimators=8)
    monkeypatch.delenv("FDX_FAULT")
    path = EnsembleCheckpointer(ck).state_path
    st = json.loads(path.read_text())
    for k in ("subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode"):
        del st["params"][k]
    path.write_text(json.dumps(st))
    assert _rank_fit(0, 1, ck=ck, resume=True, subsample=1.0, n_estimators=8) == ref
    # ... but not as a subsampled run
    with pytest.raises(RuntimeError, match="different parameters"):
        _rank_fit(0, 1, ck=ck, resume=True, subsample=0.5, n_estimators=8)


# ------------------------------------------------------------------------------- 7. API
def test_estimator_parameter_round_trip(tmp_path):
    est = SparkXGBClassifier(subsample=0.5, sampling_method="uniform", **EST_KW)
    assert est.getOrDefault("subsample") == 0.5 and SparkXGBClassifier().getOrDefault("subsample") == 1.0
    model = est.fit(_frame())
    assert _sig(model.trees) == _sig(fit_gbdt(_data()["vc"], _data()["yt"], GBDTParams(
        n_estimators=4, max_depth=3, seed=SEED, subsample=0.5), device="cpu").trees)
    model.save(tmp_path / "m")
    back = Params.load(tmp_path / "m")
    assert isinstance(back, SparkXGBClassifierModel) and _sig(back.trees) == _sig(model.trees)
    assert back.getOrDefault("subsample") == 0.5 and back.getOrDefault("sampling_method") == "uniform"
    est.save(tmp_path / "e")
    assert Params.load(tmp_path / "e").getOrDefault("subsample") == 0.5


def test_estimator_column_parameters_round_trip(tmp_path):
    kw = dict(subsample=0.8, colsample_bytree=0.5, colsample_bylevel=0.5, colsample_bynode=0.5)
    est = SparkXGBClassifier(**kw, **EST_KW)
    model = est.fit(_frame())
    want = fit_gbdt(_data()["vc"], _data()["yt"], GBDTParams(n_estimators=4, max_depth=3, seed=SEED, **kw), device="cpu")
    assert _sig(model.trees) == _sig(want.trees)
    model.save(tmp_path / "m")
    back = Params.load(tmp_path / "m")
    assert _sig(back.trees) == _sig(model.trees) and all(back.getOrDefault(k) == v for k, v in kw.items())
    est.save(tmp_path / "e")
    assert all(Params.load(tmp_path / "e").getOrDefault(k) == v for k, v in kw.items())
    assert all(SparkXGBClassifier().getOrDefault(k) == 1.0 for k in kw)


@pytest.mark.parametrize("name", ["subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode"])
@pytest.mark.parametrize("bad", [0.0, -0.5, 1.5, float("nan"), float("inf")])
def test_values_outside_the_unit_interval_raise(name, bad):
    d = _data()
    with pytest.raises(ValueError, match=name):
        fit_gbdt(d["vc"], d["yt"], GBDTParams(n_estimators=1, **{name: bad}), device="cpu")
    with pytest.raises(ValueError, match=name):
        SparkXGBClassifier(**{name: bad}, **EST_KW).fit(_frame(200))


def test_gradient_based_sampling_is_not_implemented():
    with pytest.raises(NotImplementedError, match="sampling_method"):
        SparkXGBClassifier(subsample=0.5, sampling_method="gradient_based", **EST_KW).fit(_frame(200))
