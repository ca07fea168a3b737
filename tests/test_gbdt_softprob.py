"""Multi-class gradient boosting (``multi:softprob``): the two kernels, the trainer, the
``xgboost.spark`` surface and persistence (README "Multi-class boosting").

The kernels are checked against NumPy statements of the contract in ``csrc/softprob.h``; the trainer
against a NumPy exact-histogram booster that shares no code with the engine (the one of
tests/test_oracles.py, one tree per class and round), against its own margins, across devices, under
row and column sampling and across gloo worlds."""
import functools
import json
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import Tree, class_ensemble_arrays, ensemble_arrays
from fraud_detection_spark_kafka_llm_amd.models import gbdt_softprob as GS
from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
from fraud_detection_spark_kafka_llm_amd.models.gbdt_softprob import fit_gbdt_softprob
from fraud_detection_spark_kafka_llm_amd.ops import native, sparse
from fraud_detection_spark_kafka_llm_amd.ops.text import ClassTreeArrays

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
LIM = sparse.softprob_limits()
MAXC = LIM["max_classes"]
H_FLOOR = np.float32(1e-16)
# error of softprob_grad's fp64 row terms against the NumPy formula, per unit of weight. The kernel
# stores fp32 only, so its fp64 terms are not observable directly: on the MI355X no output differs from
# NumPy's own fp32 rounding by a bit over 13e6 elements and the part of |g - g_np| / w beyond that
# rounding measures as 0 (profiles/r17/gbdt_softprob.md). The value is therefore that of the same
# softmax term w (p_c - [c == y]) of mlr_eval, 4 x the 5.921e-16 measured on the MI355X
# (tests/test_lr_multinomial.py ROW_TERM_TOL), never above 1e-13
ROW_TERM_TOL = min(4 * 5.921e-16, 1e-13)


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------ 1. softprob_grad
def softprob_np(M: np.ndarray, y: np.ndarray, w) -> tuple:
    """The contract of README "Multi-class boosting" in NumPy fp64: (g, h) fp32 ``[C, N]`` and the
    fp64 values before the rounding."""
    C = M.shape[0]
    mx = M.max(axis=0)
    e = np.exp(M - mx)
    S = np.zeros_like(mx)
    for c in range(C):                              # summed ascending
        S = S + e[c]
    p = e / S
    ww = np.ones_like(mx) if w is None else w.astype(np.float64)
    onehot = (np.arange(C)[:, None] == y[None, :].astype(np.int64)).astype(np.float64)
    g64 = ww * (p - onehot)
    h64 = np.maximum(((2.0 * p) * (1.0 - p)) * ww, 1e-16)
    return g64.astype(np.float32), h64.astype(np.float32), g64, h64


def grad_case(N: int, C: int, weighted: bool):
    rng = np.random.default_rng(1000 * C + N)
    M = rng.normal(0.0, 3.0, size=(C, N))
    y = rng.integers(0, C, size=N).astype(np.float32)
    forced = {}
    for i, v in enumerate((40.0, -40.0, 700.0, -700.0)):
        if i < N:
            k = i % C
            M[k, i] = v
            # +-700: the label is a class whose probability vanishes (g_y = -w)
            y[i] = (k + 1) % C if v > 0 else k
            forced[i] = (k, v)
    w = None
    if weighted:
        w = rng.choice(np.array([0.0, 0.3, 0.7, 1.1, 2.9], dtype=np.float32), size=N)
        if N > 4:
            w[4] = 0.0
    return M, y, w, forced


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_softprob_grad_equals_the_numpy_statement(C, dev):
    worst = 0.0
    for N in (1, 63, 64, 65, 255, 256, 257, 1025, 4097):
        for weighted in (False, True):
            M, y, w, forced = grad_case(N, C, weighted)
            g = torch.full((C, N), 7.0, dtype=torch.float32, device=dev)
            h = torch.full((C, N), 7.0, dtype=torch.float32, device=dev)
            sparse.softprob_grad(torch.from_numpy(M).to(dev), torch.from_numpy(y).to(dev),
                                 None if w is None else torch.from_numpy(w).to(dev), g, h)
            g, h = g.cpu().numpy(), h.cpu().numpy()
            rg, rh, g64, h64 = softprob_np(M, y, w)
            ww = np.ones(N) if w is None else w.astype(np.float64)
            # one fp32 ulp of the reference value plus the fp64 row-term error per unit of weight
            for got, ref in ((g, rg), (h, rh)):
                tol = np.spacing(np.abs(ref)).astype(np.float64) + ROW_TERM_TOL * ww[None, :]
                assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tol), (N, weighted)
            live = ww > 0
            if live.any():      # printed figure: what of |g - g_fp64| a correct fp32 rounding cannot explain
                worst = max(worst, float((np.maximum(np.abs(g - g64) - np.spacing(np.abs(rg)).astype(np.float64) / 2, 0)
                                          [:, live] / ww[live]).max()))
            # exact facts
            is_y = np.arange(C)[:, None] == y[None, :].astype(np.int64)
            assert np.all(g[is_y] <= 0) and np.all(g[~is_y] >= 0)
            assert np.all(h >= H_FLOOR)
            if w is not None:
                zero = w == 0
                assert np.all(g[:, zero] == 0) and np.array_equal(bits(h[:, zero]), bits(np.full_like(h[:, zero], H_FLOOR)))
            for i, (k, v) in forced.items():
                wi = np.float32(1.0) if w is None else w[i]
                if v == 700.0:       # every probability is 0 or 1: the hessian is the floor in every class
                    assert np.array_equal(bits(h[:, i]), bits(np.full(C, H_FLOOR))), (N, i)
                    assert bits(g[int(y[i]), i:i + 1])[0] == bits(np.array([-wi], dtype=np.float32))[0] or wi == 0
                if v == -700.0:      # the label's own probability vanishes
                    assert h[k, i] == H_FLOOR and (g[k, i] == -wi)
    print(f"softprob_grad C={C} {dev}: largest excess over the fp32 rounding {worst:.3e}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_softprob_grad_writes_exactly_the_rows_of_each_plane(C, dev):
    SENT = -12345.0
    for N in (257, 1025):
        M, y, w, _ = grad_case(N, C, True)
        buf = torch.full((2, C, N + 64), SENT, dtype=torch.float32, device=dev)
        g, h = buf[0, :, :N], buf[1, :, :N]
        assert not g.is_contiguous() and g.stride(0) == N + 64
        sparse.softprob_grad(torch.from_numpy(M).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev), g, h)
        out = buf.cpu().numpy()
        assert np.all(out[:, :, N:] == SENT)                      # every sentinel intact
        assert not np.any(out[:, :, :N] == SENT)                  # every [c, :N] written
        rg, rh, _, _ = softprob_np(M, y, w)
        np.testing.assert_allclose(out[0, :, :N], rg, rtol=2e-7, atol=1e-12)
        np.testing.assert_allclose(out[1, :, :N], rh, rtol=2e-7, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_device_row_terms_stay_within_one_ulp_of_the_host_twin(C):
    """The two exp implementations may differ in the last place of the fp64 terms: an fp32 output then
    differs by at most one ulp. The count of such elements is printed (profiles/r17/gbdt_softprob.md)."""
    differ = total = 0
    for N in (257, 4097):
        for weighted in (False, True):
            M, y, w, _ = grad_case(N, C, weighted)
            out = []
            for dev in ("cpu", "cuda:0"):
                g, h = torch.empty((C, N), device=dev), torch.empty((C, N), device=dev)
                sparse.softprob_grad(torch.from_numpy(M).to(dev), torch.from_numpy(y).to(dev),
                                     None if w is None else torch.from_numpy(w).to(dev), g, h)
                out.append((g.cpu().numpy(), h.cpu().numpy()))
            for a, b in zip(out[0], out[1]):
                assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(a)))
                differ += int((bits(a) != bits(b)).sum())
                total += a.size
    print(f"softprob_grad C={C}: {differ} of {total} fp32 outputs differ between host twin and device")


# ---------------------------------------------------------------------------------- 3. score_class_trees
def random_tree(rng, n_feat: int = 40) -> Tree:
    """A complete depth-3 tree over ``n_feat`` features (15 nodes, 8 leaves)."""
    n = 15
    internal = np.arange(n) < 7
    feat = np.where(internal, rng.integers(0, n_feat, n), -1).astype(np.int32)
    thr = np.where(internal, rng.uniform(-1.0, 3.0, n), 0.0)
    left = np.where(internal, 2 * np.arange(n) + 1, -1).astype(np.int32)
    right = np.where(internal, 2 * np.arange(n) + 2, -1).astype(np.int32)
    val = np.where(internal, 0.0, rng.uniform(-1.0, 1.0, n))
    z = np.zeros(n)
    return Tree(feat, thr, left, right, np.stack([val, np.ones(n)], 1), z, z.copy(), np.zeros(n, np.int64), val, 0)


def score_rows(rng, dtype) -> VectorColumn:
    """Rows of 0, 1 and 65 stored entries (and a few between) over 200 features."""
    indptr, idx, val = [0], [], []
    for ln in (0, 1, 65, 7, 40, 0, 13):
        ids = np.sort(rng.choice(200 if ln > 40 else 40, size=ln, replace=False))
        idx += list(ids)
        val += list(rng.uniform(-1.0, 3.0, ln))
        indptr.append(len(idx))
    return VectorColumn(200, torch.tensor(indptr, dtype=torch.int64), torch.tensor(idx, dtype=torch.int32),
                        torch.tensor(np.asarray(val), dtype=dtype))


def class_scores_np(vc: VectorColumn, trees, tree_class, C: int, cmp_less: bool):
    """Lane order of csrc/softprob.h: (raw [N, C], per class (leaf values taken, per row))."""
    ip, ix, v = (t.numpy() for t in vc.csr())
    n = len(ip) - 1
    out = np.zeros((n, C))
    taken = [[[] for _ in range(C)] for _ in range(n)]
    for r in range(n):
        x = dict(zip(ix[ip[r]:ip[r + 1]].tolist(), v[ip[r]:ip[r + 1]].astype(np.float64).tolist()))
        part = np.zeros((64, C))
        for t, tr in enumerate(trees):
            leaf = float(tr.stats[tr.leaf_of(x, cmp_less), 0])
            part[t & 63, tree_class[t]] += leaf
            taken[r][tree_class[t]].append(leaf)
        o = 32
        while o:
            part[:o] = part[:o] + part[o:2 * o]
            o >>= 1
        out[r] = part[0]
    return out, taken


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("C", [2, 3, MAXC])
def test_score_class_trees_bitwise_equals_the_lane_order_oracle(C, dev):
    rng = np.random.default_rng(77 + C)
    for T in (C, 63, 64, 65, 129, 193):
        trees = [random_tree(rng) for _ in range(T)]
        round_robin = np.arange(T) % C
        shuffled = rng.integers(0, C - 1, size=T)            # class C - 1 owns no tree
        for tree_class in (round_robin, shuffled):
            for dtype in (torch.float32, torch.float64):
                vc = score_rows(rng, dtype)
                for cmp_less in (True, False):
                    arr = class_ensemble_arrays(trees, tree_class, C, cmp_less=cmp_less)
                    assert isinstance(arr, ClassTreeArrays) and arr.num_trees == T
                    want, taken = class_scores_np(vc, trees, tree_class, C, cmp_less)
                    for threads in ((1, 7) if dev == "cpu" else (0,)):
                        got = sparse.score_class_trees(vc.to(dev), arr, threads=threads).cpu().numpy()
                        assert got.shape == (len(vc), C)
                        assert np.array_equal(bits(got), bits(want)), (T, dtype, cmp_less, threads)
                    if tree_class is shuffled:
                        assert np.all(bits(got[:, C - 1]) == 0)             # exactly +0.0
                    for r in range(len(vc)):
                        for c in range(C):
                            vals = taken[r][c]
                            bound = max(len(vals) - 1, 0) * 2.0 ** -53 * sum(abs(x) for x in vals)
                            assert abs(got[r, c] - math.fsum(vals)) <= bound


def test_kernel_ops_validate_before_any_launch(monkeypatch):
    lib = native.lib()

    def boom(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(lib, "softprob_grad", boom)
    monkeypatch.setattr(lib, "score_class_trees", boom)
    f64, f32 = torch.float64, torch.float32

    def grad(C=3, N=10, yn=None, wn=None, gs=None, hs=None, gdt=f32):
        yn, wn = N if yn is None else yn, N if wn is None else wn
        return sparse.softprob_grad(torch.zeros((C, N), dtype=f64), torch.zeros(yn, dtype=f32), torch.ones(wn, dtype=f32),
                                    torch.zeros(gs or (C, N), dtype=gdt), torch.zeros(hs or (C, N), dtype=f32))

    for kw in (dict(C=1), dict(C=MAXC + 1), dict(yn=9), dict(wn=11), dict(gs=(3, 9)), dict(hs=(2, 10)), dict(gdt=f64)):
        with pytest.raises(ValueError):
            grad(**kw)
    with pytest.raises(ValueError):            # planes whose rows are not contiguous
        sparse.softprob_grad(torch.zeros((3, 10), dtype=f64), torch.zeros(10), None,
                             torch.zeros((10, 3)).t(), torch.zeros((3, 10)))
    rng = np.random.default_rng(5)
    trees = [random_tree(rng) for _ in range(4)]
    vc = score_rows(rng, f64)
    for tc, C in (([0, 1, 2, 3], 3), ([0, -1, 1, 0], 3), ([0, 1, 0, 1], 1), ([0, 1, 0, 1], MAXC + 1)):
        with pytest.raises(ValueError):
            sparse.score_class_trees(vc, class_ensemble_arrays(trees, tc, C))
    with pytest.raises(ValueError, match="one entry per tree"):
        class_ensemble_arrays(trees, [0, 1, 2], 3)
    small = VectorColumn(20, torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=f64))
    with pytest.raises(ValueError, match="beyond the feature space"):
        sparse.score_class_trees(small, class_ensemble_arrays(trees, [0, 1, 2, 0], 3))
    with pytest.raises(TypeError):
        sparse.score_class_trees(vc, ensemble_arrays(trees, "value"))
    assert set(LIM) >= {"max_classes", "block", "wave"} and LIM["wave"] == 64 and MAXC == 8


def test_softprob_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--softprob-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "softprob selftest ok" in res.stdout


# ------------------------------------------------------------------------------------------ 6. the oracle
def _csr_vc(X: np.ndarray) -> VectorColumn:
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(1))]).astype(np.int64)
    r, c = np.nonzero(nz)
    return VectorColumn(X.shape[1], torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int32)),
                        torch.from_numpy(X[r, c].astype(np.float64)))


@functools.lru_cache(maxsize=None)
def int_corpus(n: int = 3000, seed: int = 11):
    """tests/test_oracles.py's integer features (value ranges of 9 .. 24 distinct values, zero
    included, some negative) plus an eleventh, and a noisy non-linear label of 3 classes."""
    rng = np.random.default_rng(seed)
    F = 11
    X = np.zeros((n, F))
    for f in range(F):
        lo = -(f % 4)
        hi = 8 + 2 * f if f < 8 else 12
        vals = rng.integers(lo, hi, n)
        keep = rng.random(n) < (0.55 + 0.04 * f)
        X[:, f] = np.where(keep, vals, 0)
    score = (1.3 * (X[:, 0] > 3) + 0.9 * (X[:, 2] * X[:, 5] > 20) - 0.8 * (X[:, 7] < 2) + 0.05 * X[:, 9]
             + 0.4 * np.sin(X[:, 4]) + 0.1 * X[:, 10]) + rng.normal(0, 0.6, n)
    y = (score > 0.4).astype(np.float32) + (score > 1.6).astype(np.float32)
    w = rng.choice(np.array([0.5, 1.0, 2.5], dtype=np.float32), size=n)
    assert set(np.unique(y)) == {0.0, 1.0, 2.0}
    return X, y, w


def _quant_exponent(m: float) -> int:
    if not m > 0:
        return 0
    return 30 - math.frexp(m)[1]


def _oracle_tree(Xb, thr_vals, g, h, params, depth_max):
    """One depth-wise tree on exact integer sums; returns (per-row leaf value, list of leaves)."""
    k0 = _quant_exponent(float(np.abs(g.astype(np.float64)).max()))
    k1 = _quant_exponent(float(np.abs(h.astype(np.float64)).max()))
    q0 = np.rint(np.ldexp(g.astype(np.float64), k0)).astype(np.int64)
    q1 = np.rint(np.ldexp(h.astype(np.float64), k1)).astype(np.int64)
    s0, s1 = math.ldexp(1.0, -k0), math.ldexp(1.0, -k1)
    lam, mcw = params.reg_lambda, params.min_child_weight
    n, F = Xb.shape
    node_of = np.zeros(n, dtype=np.int64)
    leaf_value = np.zeros(n)
    nodes = [(0, 0)]        # (node id, depth)
    next_id = 1
    leaves = []
    while nodes:
        nid, d = nodes.pop(0)
        rows = np.nonzero(node_of == nid)[0]
        T0, T1 = int(q0[rows].sum()), int(q1[rows].sum())
        G, H = T0 * s0, T1 * s1
        best = None
        if d < depth_max:
            parent = G * G / (H + lam)
            for f in range(F):
                nb = len(thr_vals[f])
                a0 = np.zeros(nb, dtype=np.int64)
                a1 = np.zeros(nb, dtype=np.int64)
                np.add.at(a0, Xb[rows, f], q0[rows])
                np.add.at(a1, Xb[rows, f], q1[rows])
                l0 = l1 = 0
                for b in range(nb - 1):
                    l0 += int(a0[b])
                    l1 += int(a1[b])
                    L0, L1 = l0 * s0, l1 * s1
                    R0, R1 = (T0 - l0) * s0, (T1 - l1) * s1
                    if L1 < mcw or R1 < mcw:
                        continue
                    gain = L0 * L0 / (L1 + lam) + R0 * R0 / (R1 + lam) - parent
                    if best is None or gain > best[0]:
                        best = (gain, f, b)
        if best is not None and best[0] > max(params.gamma, 1e-6):
            _, f, b = best
            left = rows[Xb[rows, f] <= b]
            right = rows[Xb[rows, f] > b]
            node_of[left], node_of[right] = next_id, next_id + 1
            nodes += [(next_id, d + 1), (next_id + 1, d + 1)]
            next_id += 2
            continue
        w = -G / (H + lam)
        v = params.learning_rate * w
        leaf_value[rows] = v
        leaves.append(v)
    return leaf_value, leaves


def tree_values(vc, tree) -> torch.Tensor:
    """One tree's value per row, as the resume path of fit_gbdt scores it."""
    return sparse.score_csr(vc, ensemble_arrays([tree], "value", cmp_less=False))[:, 0]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("gamma,mcw", [(0.5, 2.0), (30.0, 40.0)])
def test_softprob_gbdt_equals_numpy_exact_histogram_oracle(gamma, mcw, weighted, dev):
    X, y, w = int_corpus()
    C = 3
    w = w if weighted else None
    thr_vals = [np.unique(X[:, f]) for f in range(X.shape[1])]
    Xb = np.stack([np.searchsorted(thr_vals[f], X[:, f]) for f in range(X.shape[1])], 1)
    params = GBDTParams(n_estimators=3, max_depth=3, learning_rate=0.3, reg_lambda=1.0, gamma=gamma,
                        min_child_weight=mcw, max_bin=64)
    vc = _csr_vc(X)
    ours = fit_gbdt_softprob(vc, torch.from_numpy(y), params, device=dev, weights=w)
    assert ours.num_class == C and len(ours.trees) == 3 * C and ours.base_margin == 0.5
    assert ours.num_features == X.shape[1] and ours.train_seconds > 0 and ours.margin is None
    M = np.full((C, len(y)), 0.5)
    for t in range(params.n_estimators):
        g, h, _, _ = softprob_np(M, y, w)
        new = M.copy()
        for c in range(C):                          # all C trees see the round-start margins
            tree = ours.trees[t * C + c]            # order (t, c)
            ov, leaves = _oracle_tree(Xb, thr_vals, g[c], h[c], params, params.max_depth)
            got = tree_values(vc, tree).numpy()
            np.testing.assert_allclose(got, ov, rtol=0, atol=1e-12, err_msg=f"tree ({t}, {c})")
            ours_leaves = sorted(float(tree.stats[i, 0]) for i in range(tree.num_nodes) if tree.feature[i] < 0)
            np.testing.assert_allclose(ours_leaves, sorted(leaves), rtol=0, atol=1e-12)
            new[c] = M[c] + ov
        M = new


# --------------------------------------------------------------------------------- 7. margin bookkeeping
@pytest.mark.parametrize("dev", DEVICES)
def test_margin_planes_are_the_class_trees_added_in_training_order(dev):
    X, y, w = int_corpus()
    vc = _csr_vc(X)
    res = fit_gbdt_softprob(vc, torch.from_numpy(y), GBDTParams(n_estimators=3, max_depth=3, max_bin=64), device=dev,
                            weights=w, return_margin=True)
    C = res.num_class
    assert tuple(res.margin.shape) == (C, len(y)) and res.margin.is_contiguous()
    for c in range(C):
        m = torch.full((len(y),), res.base_margin, dtype=torch.float64)
        for i, tree in enumerate(res.trees):
            if i % C == c:
                m = m + tree_values(vc, tree)
        assert np.array_equal(bits(res.margin[c].cpu().numpy()), bits(m.numpy())), c


# -------------------------------------------------------------------------------------- 8. determinism
def same_trees(a: list, b: list) -> None:
    assert len(a) == len(b)
    for ta, tb in zip(a, b):
        np.testing.assert_array_equal(ta.feature, tb.feature)
        assert np.array_equal(bits(ta.threshold), bits(tb.threshold))
        assert np.array_equal(bits(ta.stats), bits(tb.stats))       # leaf values and covers


@pytest.mark.gpu
def test_device_trees_equal_host_trees_and_repeat():
    X, y, w = int_corpus()
    p = GBDTParams(n_estimators=3, max_depth=4, max_bin=64)
    fits = [fit_gbdt_softprob(_csr_vc(X), torch.from_numpy(y), p, device=d, weights=w)
            for d in ("cpu", "cuda:0", "cuda:0")]
    same_trees(fits[0].trees, fits[1].trees)
    same_trees(fits[1].trees, fits[2].trees)


# ----------------------------------------------------------------------------------------- 9. sampling
@pytest.mark.parametrize("dev", DEVICES)
def test_sampling_keys_on_the_tree_index(dev):
    from fraud_detection_spark_kafka_llm_amd.models.rf_sampling import row_keep_mask

    X, y, w = int_corpus()
    vc = _csr_vc(X)
    p = GBDTParams(n_estimators=2, max_depth=3, max_bin=64, subsample=0.7, colsample_bytree=0.5, seed=5)
    res = fit_gbdt_softprob(vc, torch.from_numpy(y), p, device=dev, return_margin=True)
    if dev != "cpu":
        same_trees(res.trees, fit_gbdt_softprob(vc, torch.from_numpy(y), p, device="cpu").trees)
    C, N = res.num_class, len(y)
    M = torch.full((C, N), res.base_margin, dtype=torch.float64)
    yt = torch.from_numpy(y)
    for t in range(p.n_estimators):
        G, H = torch.empty((C, N)), torch.empty((C, N))
        sparse.softprob_grad(M, yt, None, G, H)              # (the margins below are the trainer's, bit for bit)
        for c in range(C):
            tree = res.trees[t * C + c]
            h = H[c].numpy().astype(np.float64)
            k1 = _quant_exponent(float(h.max()))             # the exponent covers every row, kept or not
            keep = row_keep_mask(p.seed, t * C + c, 0, N, 0.7).numpy()
            want = int(np.rint(np.ldexp(h, k1)).astype(np.int64)[keep].sum()) * math.ldexp(1.0, -k1)
            assert tree.stats[tree.root, 1] == want, (t, c)
            if C > 1 and t > 0:          # (the key t alone would keep the same rows for every class)
                other = row_keep_mask(p.seed, t, 0, N, 0.7).numpy()
                assert not np.array_equal(keep, other)
        for c in range(C):
            M[c] += tree_values(vc, res.trees[t * C + c])
    assert np.array_equal(bits(M.numpy()), bits(res.margin.cpu().numpy()))


# ------------------------------------------------------------------------------------ 10. data parallel
def dp_corpus():
    """The integer corpus ordered so that the last shard alone (worlds 2 and 3) holds class 2."""
    X, y, w = int_corpus()
    order = np.argsort(y, kind="stable")
    X, y, w = X[order], y[order], w[order]
    assert int((y == 2).sum()) < len(y) // 3
    return X, y, w


DP_PARAMS = dict(n_estimators=2, max_depth=3, max_bin=64)


def tree_bytes(trees) -> list:
    return [(t.feature.tobytes(), t.threshold.tobytes(), t.stats.tobytes()) for t in trees]


def _dp_fit(rank, world):
    from fraud_detection_spark_kafka_llm_amd.models.tree import prepare
    from fraud_detection_spark_kafka_llm_amd.parallel import dist as D
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import Collectives, shard_range

    X, y, w = dp_corpus()
    lo, hi = shard_range(len(y), rank, world)
    if rank < world - 1:
        assert y[lo:hi].max() < 2
    vc, yy = _csr_vc(X[lo:hi]), torch.from_numpy(y[lo:hi])
    D.reset_bytes()
    prepare(vc, yy, "cpu", 64, Collectives())
    prep = dict(D.CALLS)
    D.reset_bytes()
    fit_gbdt_softprob(vc, yy, GBDTParams(**{**DP_PARAMS, "n_estimators": 0}), device="cpu", weights=w[lo:hi])
    empty = dict(D.CALLS)
    D.reset_bytes()
    res = fit_gbdt_softprob(vc, yy, GBDTParams(**DP_PARAMS), device="cpu", weights=w[lo:hi])
    return tree_bytes(res.trees), res.num_class, prep, empty, dict(D.CALLS)


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_fit_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    X, y, w = dp_corpus()
    single = fit_gbdt_softprob(_csr_vc(X), torch.from_numpy(y), GBDTParams(**DP_PARAMS), device="cpu", weights=w)
    outs = spawn(_dp_fit, world, backend="gloo")
    for trees, num_class, prep, empty, full in outs:
        assert num_class == 3                       # the global label extreme, also where the shard holds 0 .. 1
        assert trees == tree_bytes(single.trees)    # bitwise
        # one MAX all-reduce for the label extreme on top of prepare's collectives, nothing else per fit
        assert empty == {**prep, "all_reduce": prep["all_reduce"] + 1}
        # per tree what a binary tree issues: one all-reduce (the quantisation's max |g|, |h|), and per
        # level at most one reduce-scatter and one all-gather
        n_trees = len(trees)
        assert full["all_reduce"] - empty["all_reduce"] == n_trees
        depth = DP_PARAMS["max_depth"]
        assert 0 < full["reduce_scatter"] - empty["reduce_scatter"] <= n_trees * depth
        assert 0 < full["all_gather"] - empty["all_gather"] <= n_trees * depth


# ------------------------------------------------------------------------------------------- 11. errors
def test_trainer_rejects_bad_input_before_prepare(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("prepare ran")

    monkeypatch.setattr(GS, "prepare", boom)
    X, y, w = int_corpus()
    vc, p = _csr_vc(X), GBDTParams(n_estimators=1, max_depth=2)
    yt = torch.from_numpy(y)
    bad_w = w.copy()
    for labels, kw in ((y + 0.5, {}), (y - 1, {}), (np.where(y == 2, 8, y), {}), (np.where(y == 2, np.nan, y), {}),
                       (y, dict(num_class=2)), (y, dict(num_class=9)), (y, dict(num_class=1)),
                       (y, dict(weights=np.where(np.arange(len(y)) == 3, -1.0, bad_w))),
                       (y, dict(weights=np.where(np.arange(len(y)) == 3, np.inf, bad_w))),
                       (y, dict(weights=bad_w[:-1]))):
        with pytest.raises(ValueError):
            fit_gbdt_softprob(vc, torch.as_tensor(labels), p, device="cpu", **kw)
    with pytest.raises(ValueError, match="subsample"):
        fit_gbdt_softprob(vc, yt, GBDTParams(subsample=0.0), device="cpu")
    for kw in (dict(eval_set=(vc, yt, None)), dict(early_stopping_rounds=3), dict(checkpoint_dir="x"), dict(resume=True),
               dict(start_trees=[]), dict(checkpoint=lambda *a: None)):
        with pytest.raises(NotImplementedError):
            fit_gbdt_softprob(vc, yt, p, device="cpu", **kw)
    with pytest.raises(AssertionError, match="prepare ran"):      # (a good call does reach prepare)
        fit_gbdt_softprob(vc, yt, p, device="cpu", weights=w, num_class=4)


def test_memory_model_counts_the_planes():
    from fraud_detection_spark_kafka_llm_amd.utils import memory

    base = memory.training_bytes(10 ** 6, 10 ** 8)
    assert memory.training_bytes(10 ** 6, 10 ** 8, num_class=0) == base
    assert memory.training_bytes(10 ** 6, 10 ** 8, num_class=3) - base == 16 * 3 * 10 ** 6


# ------------------------------------------------------------------------------------------------ API
def frame_of(X, y, w=None):
    from fraud_detection_spark_kafka_llm_amd.ml import Frame

    cols = {"features": _csr_vc(X), "label": y.astype(np.float64)}
    if w is not None:
        cols["w"] = w
    return Frame(cols)


def column(frame, name) -> np.ndarray:
    c = frame.column(name)
    return (c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)).astype(np.float64)


XGB_KW = dict(n_estimators=3, max_depth=3, max_bin=64)


@functools.lru_cache(maxsize=None)
def xgb_model():
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier

    X, y, _ = int_corpus()
    return SparkXGBClassifier(**XGB_KW).fit(frame_of(X, y))


def test_objective_routing():
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier
    from fraud_detection_spark_kafka_llm_amd.utils.config import default_device

    X, y, _ = int_corpus()
    m = xgb_model()                                   # objective not set, labels 0 .. 2
    assert m.isMulticlass and m.numClasses == 3 and m.num_class == 3 and len(m.trees) == 9
    assert m.getOrDefault("objective") == "multi:softprob"
    direct = fit_gbdt_softprob(_csr_vc(X), torch.from_numpy(y), GBDTParams(**XGB_KW), device=default_device())
    same_trees(m.trees, direct.trees)
    with pytest.raises(ValueError, match="binary:logistic"):
        SparkXGBClassifier(objective="binary:logistic", **XGB_KW).fit(frame_of(X, y))
    with pytest.raises(NotImplementedError):
        SparkXGBClassifier(objective="reg:squarederror", **XGB_KW).fit(frame_of(X, y))
    yb = (y > 0).astype(np.float32)
    two = SparkXGBClassifier(objective="multi:softprob", **XGB_KW).fit(frame_of(X, yb))
    assert two.isMulticlass and two.numClasses == 2 and len(two.trees) == 6
    out = two.transform(frame_of(X, yb))
    assert column(out, "rawPrediction").shape == column(out, "probability").shape == (len(y), 2)
    # binary labels, default objective: the existing route, bit for bit fit_gbdt's model
    b = SparkXGBClassifier(**XGB_KW).fit(frame_of(X, yb))
    ref = fit_gbdt(_csr_vc(X), torch.from_numpy(yb), GBDTParams(**XGB_KW), device=default_device())
    assert not b.isMulticlass and b.numClasses == 2 and b.num_class == 0
    same_trees(b.trees, ref.trees)
    assert b.base_margin == ref.base_margin
    for kw in (dict(validation_indicator_col="v"), dict(early_stopping_rounds=2), dict(pred_contrib_col="c"),
               dict(num_workers=2)):
        with pytest.raises(NotImplementedError):
            SparkXGBClassifier(objective="multi:softprob", **XGB_KW, **kw).fit(frame_of(X, y))


def test_transform_outputs_and_single_row_prediction():
    X, y, _ = int_corpus()
    m = xgb_model()
    out = m.transform(frame_of(X[:500], y[:500]))
    raw, prob, pred = (column(out, n) for n in ("rawPrediction", "probability", "prediction"))
    vc = _csr_vc(X[:500])
    want = sparse.score_class_trees(vc.to(out.column("rawPrediction").device), m.class_tree_scorer()).cpu().numpy() \
        + m.base_margin
    assert np.array_equal(bits(raw), bits(want)) and raw.shape == (500, 3)
    assert np.abs(prob.sum(axis=1) - 1.0).max() <= 1e-15 * 3
    e = np.exp(raw - raw.max(axis=1, keepdims=True))
    np.testing.assert_allclose(prob, e / e.sum(axis=1, keepdims=True), rtol=8 * 2.0 ** -52)
    assert np.array_equal(pred, np.argmax(prob, axis=1).astype(np.float64))
    row = {int(f): float(v) for f, v in enumerate(X[7]) if v != 0}
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import SparseVector

    sv = SparseVector(X.shape[1], sorted(row), [row[k] for k in sorted(row)])
    assert m.predict(sv) == pred[7]
    np.testing.assert_array_equal(m.predictProbability(sv).toArray(), prob[7])
    imp = m.featureImportances.toArray()
    assert imp.shape == (X.shape[1],) and abs(imp.sum() - 1.0) < 1e-12


WORDS = [[f"{name}{i}" for i in range(12)] for name in ("bank", "prize", "parcel")]
COMMON = [f"talk{i}" for i in range(40)]


@functools.lru_cache(maxsize=None)
def dialogues(C=3):
    """A synthetic dialogue frame of ``C`` kinds: common words and a few words of the row's own kind
    (as tests/test_lr_multinomial.py generates them)."""
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    rng = np.random.default_rng(41)
    n = 420
    y = rng.integers(0, C, size=n)
    texts = []
    for c in y:
        own = rng.choice(WORDS[c], size=rng.integers(1, 4))
        other = rng.choice(WORDS[(c + 1) % C], size=int(rng.random() < 0.15))
        words = np.concatenate([rng.choice(COMMON, size=rng.integers(8, 30)), own, other])
        texts.append(" ".join(rng.permutation(words)))
    raw = TextColumn(texts)
    df = Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.astype(np.float64)})
    return df.take_rows(np.arange(300)), df.take_rows(np.arange(300, n))


@functools.lru_cache(maxsize=None)
def pipeline_model():
    from fraud_detection_spark_kafka_llm_amd.ml import IDF, HashingTF, Pipeline, StopWordsRemover, Tokenizer
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifier

    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
              IDF(inputCol="raw_features", outputCol="features"),
              SparkXGBClassifier(features_col="features", label_col="labels", n_estimators=12, max_depth=3)]
    return Pipeline(stages=stages).fit(dialogues()[0])


def test_pipeline_transform_equals_staged_and_classifies():
    from fraud_detection_spark_kafka_llm_amd.ml import Frame
    from fraud_detection_spark_kafka_llm_amd.ml.evaluation import MulticlassClassificationEvaluator

    train, test = dialogues()
    model = pipeline_model()
    clf = model.stages[-1]
    assert clf.isMulticlass and clf.numClasses == 3 and clf.numFeatures == 4096 and len(clf.trees) == 36
    for df in (train, test):
        fused = model.transform(df)
        cur = df
        for s in model.stages[:-1]:
            cur = s.transform(cur)
        vc = cur.column("features")
        ip, ix, v = vc.csr()
        feats = Frame({"features": VectorColumn(vc.size, ip.clone(), ix.clone(), v.clone()), "labels": df.column("labels")})
        staged = clf.transform(feats)
        for name in ("rawPrediction", "probability", "prediction"):
            assert np.array_equal(bits(column(fused, name)), bits(column(staged, name))), name
        raw, prob, pred = (column(fused, n) for n in ("rawPrediction", "probability", "prediction"))
        assert raw.shape == prob.shape == (len(df), 3)
        assert np.abs(prob.sum(axis=1) - 1.0).max() <= 1e-15 * 3
        assert np.array_equal(pred, np.argmax(prob, axis=1).astype(np.float64))
    y = column(test, "labels")
    acc = MulticlassClassificationEvaluator(metricName="accuracy", labelCol="labels").evaluate(model.transform(test))
    majority = float(np.bincount(y.astype(np.int64)).max()) / len(y)
    print(f"held-out accuracy {acc:.4f} on 3 classes (majority share {majority:.4f})")
    assert acc > majority


# ---------------------------------------------------------------------------------------- 14. persistence
def test_spark_layout_round_trip_is_bitwise(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifierModel

    X, y, _ = int_corpus()
    m = xgb_model()
    m.save(str(tmp_path / "m"))
    md = json.loads((tmp_path / "m" / "metadata" / "part-00000").read_text().splitlines()[0])
    assert md["numClasses"] == 3 and md["numTrees"] == 9
    back = SparkXGBClassifierModel.load(str(tmp_path / "m"))
    assert back.isMulticlass and back.numClasses == 3 and back.num_class == 3 and back.base_margin == m.base_margin
    f = frame_of(X[:400], y[:400])
    assert np.array_equal(bits(column(m.transform(f), "rawPrediction")), bits(column(back.transform(f), "rawPrediction")))
    booster = json.loads((tmp_path / "m" / "model" / "part-00000").read_text().splitlines()[0])
    L = booster["learner"]
    assert L["learner_model_param"]["num_class"] == "3"
    assert float(L["learner_model_param"]["base_score"]) == 0.5                   # the raw value: no sigmoid
    assert L["objective"] == {"name": "multi:softprob", "softmax_multiclass_param": {"num_class": "3"}}
    gb = L["gradient_booster"]["model"]
    assert gb["tree_info"] == [0, 1, 2] * 3 and gb["iteration_indptr"] == [0, 3, 6, 9]
    assert L["attributes"]["fdx_num_class"] == "3" and "fdx_trees" in L["attributes"] and \
        float(L["attributes"]["fdx_base_margin"]) == 0.5
    # the export without the fdx attributes loads through from_xgboost_json
    plain = SparkXGBClassifierModel.from_xgboost_json(m.to_xgboost_json())
    assert plain.num_class == 3 and plain.base_margin == 0.5 and len(plain.trees) == 9


def stump(feature: int, thr: float, lo: float, hi: float) -> dict:
    return {"base_weights": [0.0, lo, hi], "categories": [], "categories_nodes": [], "categories_segments": [],
            "categories_sizes": [], "default_left": [1, 0, 0], "id": 0, "left_children": [1, -1, -1],
            "right_children": [2, -1, -1], "loss_changes": [1.0, 0.0, 0.0], "parents": [2147483647, 0, 0],
            "split_conditions": [thr, lo, hi], "split_indices": [feature, 0, 0], "split_type": [0, 0, 0],
            "sum_hessian": [10.0, 4.0, 6.0],
            "tree_param": {"num_deleted": "0", "num_feature": "4", "num_nodes": "3", "size_leaf_vector": "1"}}


def test_hand_written_three_class_booster_loads_and_scores(tmp_path):
    """2 rounds of depth-1 trees, written as xgboost writes them (no fdx_* attributes)."""
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifierModel

    spec = [(0, 1.5, -0.25, 0.5), (1, 0.5, 0.125, -0.75), (2, 2.5, 0.3, -0.1),
            (3, 0.5, -0.6, 0.2), (0, 2.5, 0.05, 0.7), (1, 1.5, -0.4, 0.9)]
    trees = [dict(stump(*s), id=i) for i, s in enumerate(spec)]
    booster = {"learner": {"attributes": {}, "feature_names": [], "feature_types": [],
                           "gradient_booster": {"model": {"gbtree_model_param": {"num_parallel_tree": "1", "num_trees": "6"},
                                                          "iteration_indptr": [0, 3, 6], "tree_info": [0, 1, 2, 0, 1, 2],
                                                          "trees": trees}, "name": "gbtree"},
                           "learner_model_param": {"base_score": "2.5E-1", "boost_from_average": "1", "num_class": "3",
                                                   "num_feature": "4", "num_target": "1"},
                           "objective": {"name": "multi:softprob", "softmax_multiclass_param": {"num_class": "3"}}},
               "version": [2, 0, 3]}
    path = tmp_path / "booster.json"
    path.write_text(json.dumps(booster))
    m = SparkXGBClassifierModel.from_xgboost_json(path)
    assert m.num_class == 3 and m.numClasses == 3 and m.base_margin == 0.25 and m.numFeatures == 4
    rng = np.random.default_rng(3)
    X = rng.integers(0, 4, size=(50, 4)).astype(np.float64)
    want = np.full((50, 3), 0.25)
    for i, (f, thr, lo, hi) in enumerate(spec):             # xgboost: x < split_condition goes left
        want[:, i % 3] += np.where(X[:, f] < thr, lo, hi)
    raw = column(m.transform(frame_of(X, np.zeros(50))), "rawPrediction")
    np.testing.assert_allclose(raw, want, rtol=0, atol=1e-15)
    # and through the Spark layout's reader (model/part-00000 as xgboost.spark writes it)
    m.save(str(tmp_path / "m"))
    part = tmp_path / "m" / "model" / "part-00000"
    part.write_text(json.dumps(booster) + "\n")
    back = SparkXGBClassifierModel.load(str(tmp_path / "m"))
    assert back.num_class == 3 and np.array_equal(column(back.transform(frame_of(X, np.zeros(50))), "rawPrediction"), raw)


def test_binary_model_files_do_not_change(tmp_path):
    """A binary model writes what a model built with the multi-class attributes never set writes."""
    from fraud_detection_spark_kafka_llm_amd.ml.xgboost import SparkXGBClassifierModel

    X, y, _ = int_corpus()
    yb = (y > 0).astype(np.float32)
    res = fit_gbdt(_csr_vc(X), torch.from_numpy(yb), GBDTParams(**XGB_KW), device="cpu")
    a = SparkXGBClassifierModel(res.trees, res.num_features, res.base_margin, uid="SparkXGBClassifierModel_x")
    b = SparkXGBClassifierModel(res.trees, res.num_features, res.base_margin, uid="SparkXGBClassifierModel_x")
    for name in ("num_class", "numClasses", "_tree_class", "_class_arrays"):
        delattr(b, name)                            # as a model from before this feature
    assert json.dumps(a.to_xgboost_json()) == json.dumps(b.to_xgboost_json())
    j = a.to_xgboost_json()["learner"]
    assert j["learner_model_param"]["num_class"] == "0" and j["objective"]["name"] == "binary:logistic"
    assert j["gradient_booster"]["model"]["tree_info"] == [0] * 3
    a.save(str(tmp_path / "a"))
    b.save(str(tmp_path / "b"))
    for rel in ("model/part-00000", "metadata/part-00000"):
        ta, tb = (tmp_path / "a" / rel).read_text(), (tmp_path / "b" / rel).read_text()
        if rel.startswith("metadata"):              # (the write time differs)
            da, db = json.loads(ta), json.loads(tb)
            da.pop("timestamp"), db.pop("timestamp")
            assert list(da) == list(db)
            ta, tb = json.dumps(da), json.dumps(db)
        assert ta == tb, rel
    assert json.loads((tmp_path / "a" / "metadata" / "part-00000").read_text())["numClasses"] == 2
    assert "fdx_num_class" not in json.loads((tmp_path / "a" / "model" / "part-00000").read_text())["learner"]["attributes"]


# --------------------------------------------------------------------------- 15. serving stays out of scope
def test_binary_serving_surfaces_raise_for_a_multiclass_model():
    m = xgb_model()
    X, y, _ = int_corpus()
    with pytest.raises(ValueError, match="3 classes"):
        m.scorer()
    with pytest.raises(ValueError, match="3 classes"):
        m.paths()
    with pytest.raises(NotImplementedError):
        m.contributions(frame_of(X[:5], y[:5]))
    with pytest.raises(NotImplementedError, match="fused class-tree tail"):
        m.serving_scorer()
    with pytest.raises(NotImplementedError, match="fused class-tree tail"):
        pipeline_model().compile(multiclass=True)


# ----------------------------------------------------------------------------------------------- 16. CLI
def test_train_cli_fits_a_softprob_model_on_request(tmp_path):
    from fraud_detection_spark_kafka_llm_amd import train

    common = ["--data", "", "--synthetic", "300", "--no-plots", "--num-trees", "2", "--max-depth", "2",
              "--out-dir", str(tmp_path), "--device", "cpu"]
    summary = train.main(common + ["--xgb-label-col", "labels"])
    block = summary["MultiClassXGBoost"]
    assert block["numClasses"] == 2 and block["numTrees"] == 4
    assert block["Test"]["Accuracy"] > 0.8
    saved = json.loads((tmp_path / "results.json").read_text())["metrics"]["MultiClassXGBoost"]
    assert saved == block
