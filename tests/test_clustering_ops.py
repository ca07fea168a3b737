"""The ops behind BisectingKMeans and the silhouette (csrc/clu*.{h,hip,cpp}, ops.sparse.km_group_step /
sil_score). The oracles below write the contracts of the README's "Bisecting KMeans and silhouette"
section in NumPy: the squared norm and the dots of a row in the lane order (lane l adds entries l,
l + 64, ... ascending, then halving adds), one fp64 operation per step of the row terms, one
ties-to-even rounding per term and Python integers for the sums. Sums, assignments, distances and
coefficients are compared bit for bit."""
import functools
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ops import sparse

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
F = 300
EDGE_LENS = [0, 1, 63, 64, 65, 130]
CHUNK = 4                                             # chunk_rows of the small cases
K_E, KW_E, KC_E, KS_E = 30, 35, 20, 33                # scale exponents of the op-level tests
MEASURES = ["euclidean", "cosine"]


# ---------------------------------------------------------------------------------------------- helpers
def lane_sum_cols(T: np.ndarray) -> np.ndarray:
    """Column sums of T [m, C] in the lane order: lane l adds rows l, l + 64, ... ascending, then
    v[:32] + v[32:], v[:16] + v[16:], ..."""
    m, C = T.shape
    pad = np.zeros(((m + 63) // 64 * 64, C))
    pad[:m] = T
    p = np.zeros((64, C))
    for blk in pad.reshape(-1, 64, C):
        p = p + blk
    while p.shape[0] > 1:
        h = p.shape[0] // 2
        p = p[:h] + p[h:]
    return p[0]


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def padded(K: int) -> int:
    return (K + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def corpus(n, dtype_name, weighted, cosine=False, seed=3):
    """CSR rows (the edge lengths first; no empty row under cosine), values of both signs, weights."""
    rng = np.random.default_rng(seed + n)
    lens = np.array((EDGE_LENS + list(rng.integers(1, 13, max(n - len(EDGE_LENS), 0))))[:n])
    if cosine:
        lens[lens == 0] = 2
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    idx = np.concatenate([np.sort(rng.choice(F, size=m, replace=False)) for m in lens] + [[]]).astype(np.int32)
    val = (rng.uniform(0.05, 3.0, len(idx)) * rng.choice([1.0, 1.0, 1.0, -1.0], len(idx))).astype(np.dtype(dtype_name))
    w = rng.uniform(0.3, 1.9, n) if weighted else None
    return (indptr, idx, val), w


@functools.lru_cache(maxsize=None)
def centers(K, cosine=False, seed=5):
    """CT [F, Kp] (padding columns zero; cosine: unit columns) and cn [Kp]."""
    rng = np.random.default_rng(seed + K)
    CT = np.zeros((F, padded(K)))
    CT[:, :K] = rng.uniform(-0.5, 2.0, (F, K)) * (rng.random((F, K)) < 0.3)
    if cosine:
        CT[:, :K] /= np.sqrt((CT[:, :K] ** 2).sum(0))
    return CT, (CT * CT).sum(0)


def to_vc(csr, dev, size=F) -> VectorColumn:
    ip, ix, v = csr
    return VectorColumn(size, *(torch.from_numpy(np.array(a)).to(dev) for a in (ip, ix, v)))


def t64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def row_is_bad(x, f, wr, measure):
    """km_step's bad-row cases; returns (bad, xn)."""
    if not (np.isfinite(wr) and wr > 0) or np.any((f < 0) | (f >= F)) or not np.all(np.isfinite(x)):
        return True, 0.0
    with np.errstate(over="ignore"):
        xn = lane_sum_cols((x * x)[:, None])[0]
    return (not np.isfinite(xn)) or (measure == "cosine" and xn == 0.0), xn


def groups_of(n, G, seed=17, skip_every=3):
    """Groups 0 .. G - 1 by turns (every group that fits takes a row), every skip_every-th row skipped."""
    g = (np.arange(n) * 7 + seed) % G
    g[1::skip_every] = -1
    return g.astype(np.int32)


# ---------------------------------------------------------------------------------------------- km_group_step
def oracle_group(csr, w, group, W, G, CT, cn, measure, k=K_E, kw=KW_E, kc=KC_E):
    """(S [K, F], Wq [K], cnt [K], costq [K], flag, assign [n], dist [n]); the sums with Python integers."""
    ip, ix, v = csr
    n, K = len(ip) - 1, max(2, W * G)
    S = [[0] * F for _ in range(K)]
    Wq, cnt, costq, flag = [0] * K, [0] * K, [0] * K, 0
    assign, dist = np.full(n, -1, dtype=np.int32), np.zeros(n)
    for r in range(n):
        g = int(group[r])
        if g < 0:
            continue
        if g >= G:
            flag = 1
            continue
        x, f = v[ip[r]:ip[r + 1]].astype(np.float64), ix[ip[r]:ip[r + 1]]
        wr = 1.0 if w is None else float(w[r])
        bad, xn = row_is_bad(x, f, wr, measure)
        if bad:
            flag = 1
            continue
        cols = slice(W * g, W * g + W)
        dots = lane_sum_cols(x[:, None] * CT[f, cols])
        if measure == "cosine":
            nrm = np.sqrt(xn)
            d, s = 1.0 - dots / nrm, wr / nrm
        else:
            d, s = np.maximum((xn + cn[cols]) - 2.0 * dots, 0.0), wr
        a = 1 if W == 2 and d[1] < d[0] else 0               # the left child wins ties
        c = W * g + a
        assign[r], dist[r] = c, d[a]
        Wq[c] += int(np.rint(np.ldexp(wr, kw)))
        cnt[c] += 1
        costq[c] += int(np.rint(np.ldexp(wr * d[a], kc)))
        for fj, q in zip(f, np.rint(np.ldexp(s * x, k))):
            S[c][fj] += int(q)
    assert all(abs(q) < 2 ** 61 for row in S for q in row)
    as64 = lambda a: np.array(a, dtype=np.int64)      # noqa: E731
    return as64(S), as64(Wq), as64(cnt), as64(costq), flag, assign, dist


def run_group(csr, w, group, W, G, CT, cn, measure, dev, sums=True, **kw_):
    blk = sparse.km_group_step(to_vc(csr, dev), torch.from_numpy(np.asarray(group)), W, G, t64(CT, dev), t64(cn, dev),
                               measure, K_E, KW_E, KC_E, weights=None if w is None else torch.from_numpy(w), sums=sums,
                               want_rows=True, check=False, **kw_)
    assert blk.block.dtype == torch.int64 and blk.assign.dtype == torch.int32 and blk.dist.dtype == torch.float64
    assert blk.K == max(2, W * G) and blk.block.numel() == (blk.K * F if sums else 0) + 3 * blk.K + 1
    S = blk.S.cpu().numpy() if sums else None
    return (S, blk.Wq.cpu().numpy(), blk.cnt.cpu().numpy(), blk.costq.cpu().numpy(), blk.flag, blk.assign.cpu().numpy(),
            blk.dist.cpu().numpy())


def same_group(got, want) -> None:
    for g, t, name in zip(got, want, ("S", "Wq", "cnt", "costq", "flag", "assign", "dist")):
        if name == "dist":
            assert np.array_equal(bits(g), bits(t)), name
        elif name == "flag":
            assert g == t, name
        elif g is not None:
            assert np.array_equal(g, t), name


def check_group(n, W, G, measure, dtype_name, weighted, dev, **kw_):
    csr, w = corpus(n, dtype_name, weighted, measure == "cosine")
    CT, cn = centers(max(2, W * G), measure == "cosine")
    group = groups_of(n, G)
    want = oracle_group(csr, w, group, W, G, CT, cn, measure)
    assert want[4] == 0
    same_group(run_group(csr, w, group, W, G, CT, cn, measure, dev, **kw_), want)
    return want


def test_limits_are_exported():
    lim = sparse.clu_limits()
    assert lim["max_k"] == 64 and lim["max_width"] == 2 and lim["tile"] == 8 and lim["k_max"] == 40
    assert lim["max_table_bytes"] + 3 * 64 * 8 <= 64 * 1024           # the table and the three [64] sums fit 64 KiB


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("W,G", [(1, 1), (1, 2), (1, 9), (1, 64), (2, 1), (2, 4), (2, 5), (2, 32)])
def test_group_step_equals_the_oracle(W, G, measure, dtype_name, weighted, dev):
    want = check_group(2 * CHUNK + 3, W, G, measure, dtype_name, weighted, dev, chunk_rows=CHUNK)
    assert (want[5] == -1).sum() >= 3 and (want[5] >= 0).sum() >= 6       # skipped rows among live ones


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_group_step_equals_the_oracle_around_the_row_chunk(n, measure, dev):
    check_group(n, 2, 5, measure, "float64", True, dev, chunk_rows=CHUNK)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_group_step_equals_the_oracle_with_the_default_chunk(measure, dev):
    want = check_group(140, 2, 5, measure, "float32", True, dev)
    assert len(set(want[5].tolist())) > 6 and {int(c) % 2 for c in want[5] if c >= 0} == {0, 1}   # both children win rows


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("W", [1, 2])
def test_a_whole_chunk_of_skipped_rows(W, dev):
    csr, w = corpus(3 * CHUNK + 1, "float64", True)
    CT, cn = centers(8)
    group = groups_of(3 * CHUNK + 1, 8 // W, skip_every=5)
    group[CHUNK:2 * CHUNK] = -1                            # the second workgroup has nothing to do
    want = oracle_group(csr, w, group, W, 8 // W, CT, cn, "euclidean")
    same_group(run_group(csr, w, group, W, 8 // W, CT, cn, "euclidean", dev, chunk_rows=CHUNK), want)
    none = np.full_like(group, -1)
    got = run_group(csr, w, none, W, 8 // W, CT, cn, "euclidean", dev, chunk_rows=CHUNK)
    assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any() and got[4] == 0
    assert np.all(got[5] == -1) and np.all(bits(got[6]) == 0)


@pytest.mark.parametrize("dev", DEVICES)
def test_a_skipped_row_is_not_read(dev):
    """Only group[r] of a skipped row is read: its bad weight, value and feature id set no flag."""
    (ip, ix, v), w = corpus(2 * CHUNK + 3, "float64", True)
    ix, v, w = ix.copy(), v.copy(), w.copy()
    group = groups_of(2 * CHUNK + 3, 4)
    group[[2, 3, 5]] = -1
    ix[ip[2]] = F + 9
    v[ip[3]] = float("nan")
    w[5] = -1.0
    CT, cn = centers(8)
    got = run_group((ip, ix, v), w, group, 2, 4, CT, cn, "euclidean", dev, chunk_rows=CHUNK)
    assert got[4] == 0 and got[2].sum() == (group >= 0).sum()
    same_group(got, oracle_group((ip, ix, v), w, group, 2, 4, CT, cn, "euclidean"))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_identical_children_every_row_goes_left(measure, dev):
    csr, w = corpus(140, "float64", True, measure == "cosine")
    CT, cn = (a.copy() for a in centers(10, measure == "cosine"))
    CT[:, 1::2], cn[1::2] = CT[:, 0::2], cn[0::2]
    CT[:, 10:], cn[10:] = 0.0, 0.0
    group = groups_of(140, 5)
    S, Wq, cnt, costq, flag, assign, _ = run_group(csr, w, group, 2, 5, CT, cn, measure, dev)
    assert flag == 0 and not cnt[1::2].any() and not Wq[1::2].any() and not costq[1::2].any() and not S[1::2].any()
    assert np.all(cnt[0:10:2] > 0) and np.array_equal(assign[group >= 0], 2 * group[group >= 0])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("W,G", [(1, 2), (1, 64), (2, 1), (2, 32)])
def test_group_hot_set_chunk_and_threads_change_no_bit(W, G, dev):
    csr, w = corpus(140, "float32", True)
    K = max(2, W * G)
    CT, cn = centers(K)
    group = groups_of(140, G)
    want = oracle_group(csr, w, group, W, G, CT, cn, "euclidean")
    slots = sparse.clu_limits()["max_table_bytes"] // (8 * K)
    picked = np.unique(csr[1])[::3][:slots]               # hand-picked: every third feature that occurs
    for hot in (None, [], picked[:5], picked, np.arange(min(slots, F))):
        same_group(run_group(csr, w, group, W, G, CT, cn, "euclidean", dev, hot=hot), want)
    for chunk_rows in (1, 5, 64):
        same_group(run_group(csr, w, group, W, G, CT, cn, "euclidean", dev, chunk_rows=chunk_rows), want)
    for threads in (1, 2, 7):
        same_group(run_group(csr, w, group, W, G, CT, cn, "euclidean", dev, threads=threads), want)
    if dev != "cpu" and (slots + 1) <= F:
        with pytest.raises(ValueError):
            run_group(csr, w, group, W, G, CT, cn, "euclidean", dev, hot=np.arange(slots + 1))


def test_host_threads_change_no_bit_with_rows_for_every_thread():
    csr, w = corpus(1800, "float64", True)                # 256 rows a thread: seven threads get rows
    CT, cn = centers(10)
    group = groups_of(1800, 5)
    ref = run_group(csr, w, group, 2, 5, CT, cn, "euclidean", "cpu", threads=1)
    labels, stats = labels_of(1800, 9), None
    stats = cluster_stats(csr, w, labels, 9, "euclidean")
    sref = run_sil(csr, w, labels, 9, stats, "euclidean", "cpu", threads=1)
    for threads in (2, 7):
        same_group(run_group(csr, w, group, 2, 5, CT, cn, "euclidean", "cpu", threads=threads), ref)
        same_sil(run_sil(csr, w, labels, 9, stats, "euclidean", "cpu", threads=threads), sref)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("W,G", [(1, 9), (2, 1), (2, 32)])
def test_group_assign_only_equals_the_full_pass(W, G, measure, dev):
    csr, w = corpus(140, "float32", True, measure == "cosine")
    CT, cn = centers(max(2, W * G), measure == "cosine")
    group = groups_of(140, G)
    full = run_group(csr, w, group, W, G, CT, cn, measure, dev)
    only = run_group(csr, w, group, W, G, CT, cn, measure, dev, sums=False)
    assert only[0] is None
    same_group(only, full)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
def test_width_one_is_a_class_given_accumulation_and_zero_centers_give_psi(weighted, dev):
    """W = 1 with group = labels sums by class; with CT = 0 and cn = 0 under the euclidean measure
    d = xn, so costq[c] is the sum of rint(w |x|^2 2^kc) over the rows of class c."""
    csr, w = corpus(140, "float64", weighted)
    ip, ix, v = csr
    labels = labels_of(140, 9)
    zero = np.zeros((F, 16))
    S, Wq, cnt, costq, flag, assign, dist = run_group(csr, w, labels, 1, 9, zero, np.zeros(16), "euclidean", dev)
    assert flag == 0 and np.array_equal(assign, labels)
    psiq, Sq = [0] * 9, np.zeros((9, F), dtype=np.int64)
    for r in range(140):
        x = v[ip[r]:ip[r + 1]]
        wr = 1.0 if w is None else float(w[r])
        xn = lane_sum_cols((x * x)[:, None])[0]
        assert bits(dist[r]) == bits(xn)
        psiq[labels[r]] += int(np.rint(np.ldexp(wr * xn, KC_E)))
        np.add.at(Sq[labels[r]], ix[ip[r]:ip[r + 1]], np.rint(np.ldexp(wr * x, K_E)).astype(np.int64))
    assert costq.tolist() == psiq and np.array_equal(S, Sq) and np.array_equal(cnt, np.bincount(labels, minlength=9))


def changed(a, i, x):
    b = a.copy()
    b[i] = x
    return b


@pytest.mark.parametrize("dev", DEVICES)
def test_group_bad_input_sets_the_flag_and_adds_nothing(dev):
    (ip, ix, v), w = corpus(140, "float64", True, cosine=True)
    CT, cn = centers(10)
    group = groups_of(140, 5)
    live = [int(r) for r in np.nonzero(group >= 0)[0][[2, 11, 30]]]

    def check(idx=ix, val=v, weights=w, grp=group, measure="euclidean", row=live[0]):
        got = run_group((ip, idx, val), weights, grp, 2, 5, CT, cn, measure, dev, chunk_rows=CHUNK)
        clean = run_group((ip, ix, v), w, changed(group, row, -1), 2, 5, CT, cn, measure, dev, chunk_rows=CHUNK)
        assert got[4] == 1 and clean[4] == 0 and got[5][row] == -1 and got[6][row] == 0.0
        same_group(got[:4] + (0,) + got[5:], clean)        # the sums are those of the data without the row
        same_group(got, oracle_group((ip, idx, val), weights, grp, 2, 5, CT, cn, measure))
        with pytest.raises(ValueError):
            sparse.km_group_step(to_vc((ip, idx, val), dev), torch.from_numpy(grp), 2, 5, t64(CT, dev), t64(cn, dev),
                                 measure, K_E, KW_E, KC_E, weights=torch.from_numpy(weights))

    for bad in (F, -1, 2 ** 31 - 1):
        check(idx=changed(ix, int(ip[live[0]]), bad))
    for bad in (float("nan"), float("inf"), -float("inf"), 1e200):            # 1e200: the squared norm overflows
        check(val=changed(v, int(ip[live[1]]), bad), row=live[1])
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        check(weights=changed(w, live[2], bad), row=live[2])
    for bad in (5, 6, 2 ** 31 - 1):
        check(grp=changed(group, live[0], bad))
    zero_row = v.copy()
    zero_row[ip[live[1]]:ip[live[1] + 1]] = 0.0
    check(val=zero_row, measure="cosine", row=live[1])
    assert run_group((ip, ix, zero_row), w, group, 2, 5, CT, cn, "euclidean", dev)[4] == 0
    if dev != "cpu":
        torch.cuda.synchronize()                           # the device run ends clean


@pytest.mark.parametrize("dev", DEVICES)
def test_arguments_are_checked_before_any_launch(dev):
    csr, w = corpus(11, "float64", False)
    vc = to_vc(csr, dev)
    CT, cn = (t64(a, dev) for a in centers(10))
    group = torch.from_numpy(groups_of(11, 5))
    ok = dict(vc=vc, group=group, W=2, G=5, CT=CT, cn=cn, measure="euclidean", k=K_E, kw=KW_E, kc=KC_E)
    assert sparse.km_group_step(**ok).flag == 0
    for bad in ({"W": 0}, {"W": 3}, {"G": 0}, {"G": 33}, {"W": 1, "G": 65}, {"measure": "manhattan"}, {"kc": 41},
                {"k": -1}, {"CT": CT[:, :8].contiguous()}, {"cn": cn[:8].contiguous()}, {"CT": CT.to(torch.float32)},
                {"group": group[:10]}, {"group": group.to(torch.float64)}, {"weights": torch.ones(10)},
                {"G": 4}):                                                     # G = 4: K = 8, CT is [F, 16]
        with pytest.raises(ValueError):
            sparse.km_group_step(**{**ok, **bad})
    labels = labels_of(11, 9)
    stats = cluster_stats(csr, w, labels, 9, "euclidean")
    MT, psi, nw, cnt = (t64(a, dev) for a in stats)
    sok = dict(vc=vc, labels=torch.from_numpy(labels), K=9, MT=MT, psi=psi, nw=nw, cnt=cnt, measure="euclidean",
               ks=KS_E, kw=KW_E)
    assert sparse.sil_score(**sok).flag == 0
    for bad in ({"K": 1}, {"K": 65}, {"K": 8}, {"measure": "l1"}, {"ks": 41}, {"kw": -1}, {"MT": MT[:, :8].contiguous()},
                {"psi": psi[:9].contiguous()}, {"nw": nw.to(torch.float32)}, {"cnt": cnt.to(torch.int64)},
                {"labels": torch.from_numpy(labels[:10])}, {"labels": torch.from_numpy(labels.astype(np.float64))},
                {"weights": torch.ones(12)}):
        with pytest.raises(ValueError):
            sparse.sil_score(**{**sok, **bad})


# ---------------------------------------------------------------------------------------------- sil_score
def labels_of(n, K, present=None, seed=23):
    """Labels by turns over the `present` clusters (default: all that fit), int32."""
    present = np.arange(K) if present is None else np.asarray(present)
    return present[(np.arange(n) * 5 + seed) % len(present)].astype(np.int32)


def cluster_stats(csr, w, labels, K, measure):
    """(MT [F, Kp], psi [Kp], nw [Kp], cnt [Kp] int32) of a labelling in plain NumPy: the op takes them
    as given."""
    ip, ix, v = csr
    n, Kp = len(ip) - 1, padded(K)
    ww = np.ones(n) if w is None else w
    MT, psi, nw, cnt = np.zeros((F, Kp)), np.zeros(Kp), np.zeros(Kp), np.zeros(Kp, dtype=np.int32)
    for r in range(n):
        x, f, c = v[ip[r]:ip[r + 1]].astype(np.float64), ix[ip[r]:ip[r + 1]], labels[r]
        xn = float((x * x).sum())
        scale = ww[r] / math.sqrt(xn) if measure == "cosine" else ww[r]
        MT[f, c] += scale * x
        psi[c] += 0.0 if measure == "cosine" else ww[r] * xn
        nw[c] += ww[r]
        cnt[c] += 1
    live = nw > 0
    MT[:, live] /= nw[live]
    psi[live] /= nw[live]
    return MT, psi, nw, cnt


def oracle_sil(csr, w, labels, K, stats, measure, ks=KS_E, kw=KW_E):
    """(silq, wq, flag, s [n], neighbour [n]); the sums with Python integers."""
    ip, ix, v = csr
    MT, psi, nw, cnt = stats
    n = len(ip) - 1
    silq = wq = flag = 0
    s_rows, nb_rows = np.zeros(n), np.full(n, -1)
    for r in range(n):
        x, f, a = v[ip[r]:ip[r + 1]].astype(np.float64), ix[ip[r]:ip[r + 1]], int(labels[r])
        wr = 1.0 if w is None else float(w[r])
        bad, xn = row_is_bad(x, f, wr, measure)
        if bad or not 0 <= a < K or not nw[a] > 0:
            flag = 1
            continue
        dots = lane_sum_cols(x[:, None] * MT[f, :K])
        with np.errstate(all="ignore"):
            D = 1.0 - dots / np.sqrt(xn) if measure == "cosine" else (xn + psi[:K]) - 2.0 * dots    # unclamped
            nb, nb_c = None, -1
            for c in range(K):
                if c != a and nw[c] > 0 and (nb is None or D[c] < nb):
                    nb, nb_c = D[c], c
            if nb is None:
                flag = 1
                continue
            if cnt[a] == 1:
                s = 0.0
            else:
                rest = nw[a] - wr
                if not rest > 0:
                    flag = 1
                    continue
                own = (D[a] * nw[a]) / rest
                s = 1.0 - own / nb if own < nb else nb / own - 1.0 if own > nb else 0.0
                if not (np.isfinite(own) and np.isfinite(nb) and np.isfinite(s)):
                    flag = 1
                    continue
        s_rows[r], nb_rows[r] = s, nb_c
        silq += int(np.rint(np.ldexp(wr * s, ks)))
        wq += int(np.rint(np.ldexp(wr, kw)))
    return silq, wq, flag, s_rows, nb_rows


def run_sil(csr, w, labels, K, stats, measure, dev, **kw_):
    MT, psi, nw, cnt = (t64(a, dev) for a in stats)
    blk = sparse.sil_score(to_vc(csr, dev), torch.from_numpy(np.asarray(labels)), K, MT, psi, nw, cnt, measure, KS_E, KW_E,
                           weights=None if w is None else torch.from_numpy(w), want_rows=True, check=False, **kw_)
    assert blk.block.dtype == torch.int64 and blk.block.numel() == 3 and blk.s.dtype == torch.float64
    return blk.silq, blk.wq, blk.flag, blk.s.cpu().numpy()


def same_sil(got, want) -> None:
    assert got[:3] == tuple(want[:3])
    assert np.array_equal(bits(got[3]), bits(want[3]))


def check_sil(n, K, measure, dtype_name, weighted, dev, present=None, **kw_):
    csr, w = corpus(n, dtype_name, weighted, measure == "cosine")
    labels = labels_of(n, K, present)
    stats = cluster_stats(csr, w, labels, K, measure)
    want = oracle_sil(csr, w, labels, K, stats, measure)
    assert want[2] == 0
    same_sil(run_sil(csr, w, labels, K, stats, measure, dev, **kw_), want)
    return want, labels, stats


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [2, 8, 9, 64])
def test_sil_score_equals_the_oracle(K, measure, dtype_name, weighted, dev):
    present = [3, 17, 40, 63] if K == 64 else None         # eleven rows: by turns over 64 every cluster is a singleton
    want, labels, stats = check_sil(2 * CHUNK + 3, K, measure, dtype_name, weighted, dev, present=present,
                                    chunk_rows=CHUNK)
    assert np.count_nonzero(want[3]) >= 2 and (K < 64 or (stats[2][:K] == 0).sum() > 40)   # K = 64: most are absent


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_sil_score_equals_the_oracle_around_the_row_chunk(n, measure, dev):
    check_sil(n, 9, measure, "float64", True, dev, present=[1, 8], chunk_rows=CHUNK)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_sil_score_equals_the_oracle_with_the_default_chunk(measure, dev):
    want, _, _ = check_sil(140, 9, measure, "float32", True, dev)
    assert (want[3] > 0).any() and (want[3] < 0).any()      # both branches of the coefficient


@pytest.mark.parametrize("dev", DEVICES)
def test_own_cluster_and_neighbour_in_different_tiles(dev):
    """Clusters 0 and 8 share a mean up to a small shift and every other mean is far: rows of cluster
    0 have their neighbour in the second tile, rows of cluster 8 in the first."""
    csr, w = corpus(140, "float64", True)
    labels = labels_of(140, 9)
    MT, psi, nw, cnt = cluster_stats(csr, w, labels, 9, "euclidean")
    rng = np.random.default_rng(4)
    MT[:, 1:8] = rng.uniform(40.0, 50.0, (F, 7))
    MT[:, 8] = MT[:, 0] * 1.01
    psi[1:8], psi[8] = (MT[:, 1:8] ** 2).sum(0), psi[0]   # the far means at their true squared distances
    stats = (MT, psi, nw, cnt)
    want = oracle_sil(csr, w, labels, 9, stats, "euclidean")
    assert want[2] == 0 and np.all(want[4][labels == 0] == 8) and np.all(want[4][labels == 8] == 0)
    assert np.all(want[4][(labels != 0) & (labels != 8)] != -1)
    same_sil(run_sil(csr, w, labels, 9, stats, "euclidean", dev), want)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_a_singleton_scores_zero_and_absent_clusters_never_compete(measure, dev):
    csr, w = corpus(140, "float64", True, measure == "cosine")
    labels = labels_of(140, 9, present=[1, 4, 8])
    labels[17] = 6                                         # the only row of cluster 6
    MT, psi, nw, cnt = cluster_stats(csr, w, labels, 9, measure)
    MT[:, [0, 2, 3, 5, 7]] = MT[:, [1]]                    # absent clusters sit on a present one: they would win
    psi[[0, 2, 3, 5, 7]] = -1e6
    want = oracle_sil(csr, w, labels, 9, (MT, psi, nw, cnt), measure)
    assert want[2] == 0 and cnt[6] == 1 and want[3][17] == 0.0 and set(want[4].tolist()) <= {1, 4, 6, 8}
    got = run_sil(csr, w, labels, 9, (MT, psi, nw, cnt), measure, dev)
    same_sil(got, want)
    assert got[3][17] == 0.0 and np.count_nonzero(got[3]) > 100


@pytest.mark.parametrize("dev", DEVICES)
def test_sil_chunk_and_threads_change_no_bit(dev):
    csr, w = corpus(140, "float32", True)
    labels = labels_of(140, 9)
    stats = cluster_stats(csr, w, labels, 9, "euclidean")
    want = oracle_sil(csr, w, labels, 9, stats, "euclidean")
    for chunk_rows in (1, 5, 64):
        same_sil(run_sil(csr, w, labels, 9, stats, "euclidean", dev, chunk_rows=chunk_rows), want)
    for threads in (1, 2, 7):
        same_sil(run_sil(csr, w, labels, 9, stats, "euclidean", dev, threads=threads), want)


@pytest.mark.parametrize("dev", DEVICES)
def test_sil_bad_input_sets_the_flag_and_adds_nothing(dev):
    (ip, ix, v), w = corpus(140, "float64", True, cosine=True)
    labels = labels_of(140, 9, present=[0, 3, 8])
    stats = cluster_stats((ip, ix, v), w, labels, 9, "euclidean")
    cstats = cluster_stats((ip, ix, v), w, labels, 9, "cosine")

    def check(row, idx=ix, val=v, weights=w, lab=labels, st=stats, measure="euclidean", whole=False):
        want = oracle_sil((ip, idx, val), weights, lab, 9, st, measure)
        got = run_sil((ip, idx, val), weights, lab, 9, st, measure, dev, chunk_rows=CHUNK)
        assert want[2] == 1 and got[3][row] == 0.0
        same_sil(got, want)
        if not whole:                                      # every other row counts: the weight sum misses this row's
            assert got[1] == sum(int(np.rint(np.ldexp(x, KW_E))) for r, x in enumerate(w) if r != row)
        MT, psi, nw, cnt = (t64(a, dev) for a in st)
        with pytest.raises(ValueError):
            sparse.sil_score(to_vc((ip, idx, val), dev), torch.from_numpy(lab), 9, MT, psi, nw, cnt, measure, KS_E, KW_E,
                             weights=torch.from_numpy(weights))

    for bad in (F, -1, 2 ** 31 - 1):
        check(20, idx=changed(ix, int(ip[20]), bad))
    for bad in (float("nan"), float("inf"), -float("inf"), 1e200):
        check(21, val=changed(v, int(ip[21]), bad))
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        check(22, weights=changed(w, 22, bad))
    for bad in (-1, 9, 64, 2 ** 31 - 1, 5):                # 5: an absent cluster
        check(23, lab=changed(labels, 23, bad))
    zero_row = v.copy()
    zero_row[ip[24]:ip[25]] = 0.0
    check(24, val=zero_row, st=cstats, measure="cosine")
    # the weight sum of a cluster does not exceed the row's: nw_a - w is not > 0
    row = int(np.nonzero(labels == 3)[0][0])
    small = tuple(a.copy() for a in stats)
    small[2][3] = w[row] * 0.5
    want = oracle_sil((ip, ix, v), w, labels, 9, small, "euclidean")
    assert want[2] == 1
    same_sil(run_sil((ip, ix, v), w, labels, 9, small, "euclidean", dev), want)
    # a coefficient that is not finite
    inf_psi = tuple(a.copy() for a in stats)
    inf_psi[1][8] = float("inf")
    want = oracle_sil((ip, ix, v), w, labels, 9, inf_psi, "euclidean")
    assert want[2] == 1 and want[1] > 0
    same_sil(run_sil((ip, ix, v), w, labels, 9, inf_psi, "euclidean", dev), want)
    # a single present cluster: no row has a neighbour
    one = np.zeros(140, dtype=np.int32)
    alone = cluster_stats((ip, ix, v), w, one, 9, "euclidean")
    check(0, lab=one, st=alone, whole=True)
    assert run_sil((ip, ix, v), w, one, 9, alone, "euclidean", dev)[:3] == (0, 0, 1)
    if dev != "cpu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- self-test
def test_clu_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--clu-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "clu_selftest: ok" in res.stdout
