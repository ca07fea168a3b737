"""KMeans (csrc/km*.{h,hip,cpp}, ops.sparse.km_step / km_centers, models/kmeans.py, ml.KMeans and its users).
The oracle below writes the contract of the README's "KMeans" section in NumPy: the squared norm and
the dots of a row in the lane order (lane l adds entries l, l + 64, ... ascending, then halving adds),
one fp64 operation per step of the row terms, one ties-to-even rounding per term and Python integers
for the sums. Sums, assignments and distances are compared bit for bit."""
import functools
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.models import kmeans as KM
from fraud_detection_spark_kafka_llm_amd.ops import sparse

DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda:0", id="device", marks=pytest.mark.gpu)]
F = 300
LIM = sparse.km_limits()
EDGE_LENS = [0, 1, 63, 64, 65, 130]
CHUNK = 4                                             # chunk_rows of the small cases
K_E, KW_E, KC_E = 30, 35, 20                          # scale exponents of the op-level tests
MEASURES = ["euclidean", "cosine"]


# ---------------------------------------------------------------------------------------------- oracle
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
    Kp = (K + 7) // 8 * 8
    CT = np.zeros((F, Kp))
    CT[:, :K] = rng.uniform(-0.5, 2.0, (F, K)) * (rng.random((F, K)) < 0.3)
    if cosine:
        CT[:, :K] /= np.sqrt((CT[:, :K] ** 2).sum(0))
    return CT, (CT * CT).sum(0)


def to_vc(csr, dev, size=F) -> VectorColumn:
    ip, ix, v = csr
    return VectorColumn(size, *(torch.from_numpy(np.array(a)).to(dev) for a in (ip, ix, v)))


def oracle_step(csr, w, CT, cn, K, measure, k=K_E, kw=KW_E, kc=KC_E):
    """(S [K, F], Wq [K], cnt [K], costq, assign [n], dist [n]); the sums with Python integers."""
    ip, ix, v = csr
    n = len(ip) - 1
    S = [[0] * F for _ in range(K)]
    Wq, cnt, costq = [0] * K, [0] * K, 0
    assign, dist = np.zeros(n, dtype=np.int32), np.zeros(n)
    for r in range(n):
        x, f = v[ip[r]:ip[r + 1]].astype(np.float64), ix[ip[r]:ip[r + 1]]
        wr = 1.0 if w is None else float(w[r])
        xn = lane_sum_cols((x * x)[:, None])[0]
        dots = lane_sum_cols(x[:, None] * CT[f, :K])
        if measure == "cosine":
            nrm = np.sqrt(xn)
            d, s = 1.0 - dots / nrm, wr / nrm
        else:
            d, s = np.maximum((xn + cn[:K]) - 2.0 * dots, 0.0), wr
        a = int(np.argmin(d))                          # the first index that attains the minimum
        assign[r], dist[r] = a, d[a]
        Wq[a] += int(np.rint(np.ldexp(wr, kw)))
        cnt[a] += 1
        costq += int(np.rint(np.ldexp(wr * d[a], kc)))
        for fj, q in zip(f, np.rint(np.ldexp(s * x, k))):
            S[a][fj] += int(q)
    assert all(abs(q) < 2 ** 61 for row in S for q in row)
    return np.array(S, dtype=np.int64), np.array(Wq, dtype=np.int64), np.array(cnt, dtype=np.int64), costq, assign, dist


def run_step(csr, w, CT, cn, K, measure, dev, sums=True, **kw_):
    blk = sparse.km_step(to_vc(csr, dev), torch.from_numpy(CT).to(dev), torch.from_numpy(cn).to(dev), K, measure,
                         K_E, KW_E, KC_E, weights=None if w is None else torch.from_numpy(w), sums=sums,
                         want_rows=True, **kw_)
    assert blk.block.dtype == torch.int64 and blk.assign.dtype == torch.int32 and blk.dist.dtype == torch.float64
    S = blk.S.cpu().numpy() if sums else None
    return S, blk.Wq.cpu().numpy(), blk.cnt.cpu().numpy(), blk.costq, blk.assign.cpu().numpy(), blk.dist.cpu().numpy()


def same(got, want) -> None:
    for g, t, name in zip(got, want, ("S", "Wq", "cnt", "costq", "assign", "dist")):
        if name == "dist":
            assert np.array_equal(bits(g), bits(t)), name
        elif name == "costq":
            assert g == t, name
        elif g is not None:
            assert np.array_equal(g, t), name


def check_step(n, K, measure, dtype_name, weighted, dev, **kw_):
    csr, w = corpus(n, dtype_name, weighted, measure == "cosine")
    CT, cn = centers(K, measure == "cosine")
    want = oracle_step(csr, w, CT, cn, K, measure)
    same(run_step(csr, w, CT, cn, K, measure, dev, **kw_), want)
    return want


# ---------------------------------------------------------------------------------------------- 1. km_step
def test_limits_are_exported():
    assert set(LIM) >= {"max_k", "tile", "chunk_rows", "table_bytes", "max_table_bytes", "k_max", "sum_bits"}
    assert LIM["max_k"] == 64 and LIM["tile"] == 8 and LIM["k_max"] == 40 and LIM["sum_bits"] == 61
    assert 0 < LIM["table_bytes"] <= LIM["max_table_bytes"] and LIM["max_table_bytes"] + (2 * 64 + 1) * 8 <= 64 * 1024


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weights"])
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [2, 8, 9, 64])
def test_step_equals_the_oracle(K, measure, dtype_name, weighted, dev):
    want = check_step(2 * CHUNK + 3, K, measure, dtype_name, weighted, dev, chunk_rows=CHUNK)
    assert len(set(want[4].tolist())) > 1                  # more than one cluster takes rows


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_step_equals_the_oracle_around_the_row_chunk(n, measure, dev):
    check_step(n, 9, measure, "float64", True, dev, chunk_rows=CHUNK)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_step_equals_the_oracle_with_the_default_chunk(measure, dev):
    check_step(140, 9, measure, "float32", True, dev)


# ---------------------------------------------------------------------------------------------- 2. order-freedom
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("K", [2, 9, 64])
def test_hot_set_chunk_and_threads_change_no_bit(K, dev):
    csr, w = corpus(140, "float32", True)
    CT, cn = centers(K)
    want = oracle_step(csr, w, CT, cn, K, "euclidean")
    slots = LIM["max_table_bytes"] // (8 * K)
    picked = np.unique(csr[1])[::3][:slots]               # hand-picked: every third feature that occurs
    for hot in (None, [], picked, np.arange(min(slots, F))):
        same(run_step(csr, w, CT, cn, K, "euclidean", dev, hot=hot), want)
    for chunk_rows in (1, 5, 64):
        same(run_step(csr, w, CT, cn, K, "euclidean", dev, chunk_rows=chunk_rows), want)
    for threads in (1, 2, 7):
        same(run_step(csr, w, CT, cn, K, "euclidean", dev, threads=threads), want)
    if dev != "cpu" and (slots + 1) <= F:
        with pytest.raises(ValueError):
            run_step(csr, w, CT, cn, K, "euclidean", dev, hot=np.arange(slots + 1))


def test_host_threads_change_no_bit_with_rows_for_every_thread():
    csr, w = corpus(1800, "float64", True)                # 256 rows a thread: seven threads get rows
    CT, cn = centers(9)
    ref = run_step(csr, w, CT, cn, 9, "euclidean", "cpu", threads=1)
    for threads in (2, 7):
        same(run_step(csr, w, CT, cn, 9, "euclidean", "cpu", threads=threads), ref)


# ---------------------------------------------------------------------------------------------- 3. ties and structure
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
def test_identical_centers_the_smaller_index_wins(measure, dev):
    csr, w = corpus(140, "float64", True, measure == "cosine")
    CT, cn = (a.copy() for a in centers(9, measure == "cosine"))
    CT[:, 5], cn[5] = CT[:, 2], cn[2]
    S, Wq, cnt, _, assign, _ = run_step(csr, w, CT, cn, 9, measure, dev)
    assert cnt[2] > 0 and cnt[5] == 0 and Wq[5] == 0 and not S[5].any() and 5 not in assign
    # the empty cluster keeps its center and does not move
    nCT, ncn, moved2 = sparse.km_centers(torch.from_numpy(S).to(dev), torch.from_numpy(Wq).to(dev),
                                         torch.from_numpy(CT).to(dev), 9, K_E, KW_E, measure)
    assert np.array_equal(bits(nCT[:, 5].cpu().numpy()), bits(CT[:, 5])) and float(moved2[5]) == 0.0
    assert float(moved2.max()) > 0.0 and not nCT[:, 9:].any() and not ncn[9:].any()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [2, 9, 64])
def test_assign_only_equals_the_full_pass(K, measure, dev):
    csr, w = corpus(140, "float32", True, measure == "cosine")
    CT, cn = centers(K, measure == "cosine")
    full = run_step(csr, w, CT, cn, K, measure, dev)
    only = run_step(csr, w, CT, cn, K, measure, dev, sums=False)
    assert only[0] is None
    same(only, full)
    pred = KM.predict_kmeans(to_vc(csr, dev), CT[:, :K].T, measure)
    if measure == "euclidean":                            # predict_kmeans takes the norms of the centers itself
        assert pred.dtype == torch.int32 and pred.shape == (140,)
    else:
        assert np.array_equal(pred.cpu().numpy(), full[4])


@pytest.mark.parametrize("dev", DEVICES)
def test_best_center_in_the_second_tile(dev):
    csr, w = corpus(2 * CHUNK + 3, "float64", False)
    CT, cn = (a.copy() for a in centers(9))
    ip, ix, v = csr
    r = 4                                                  # the row of 65 entries becomes center 8
    CT[:, 8] = 0.0
    CT[ix[ip[r]:ip[r + 1]], 8] = v[ip[r]:ip[r + 1]]
    cn[8] = (CT[:, 8] ** 2).sum()
    want = oracle_step(csr, w, CT, cn, 9, "euclidean")
    assert want[4][r] == 8 and want[2][8] >= 1
    same(run_step(csr, w, CT, cn, 9, "euclidean", dev, chunk_rows=CHUNK), want)


# ---------------------------------------------------------------------------------------------- 4. km_centers
def dyadic_weights(n, seed=9):
    return np.random.default_rng(seed).choice([0.5, 1.0, 2.0], n)      # w x and the weight sums are exact


@functools.lru_cache(maxsize=None)
def centers_case(K, measure, dev):
    csr, _ = corpus(140, "float64", False, measure == "cosine")
    w = dyadic_weights(140)
    CT, cn = centers(K, measure == "cosine")
    S, Wq, cnt, _, assign, _ = run_step(csr, w, CT, cn, K, measure, "cpu")
    out = sparse.km_centers(torch.from_numpy(S).to(dev), torch.from_numpy(Wq).to(dev), torch.from_numpy(CT).to(dev),
                            K, K_E, KW_E, measure)
    return csr, w, CT, (S, Wq, cnt, assign), tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("K", [2, 9, 64])
def test_centers_host_equals_device_and_numpy_within_the_bound(K, measure, dev):
    csr, w, CT, (S, Wq, cnt, assign), (nCT, ncn, moved2) = centers_case(K, measure, dev)
    host = centers_case(K, measure, "cpu")[4]
    for g, h in zip((nCT, ncn, moved2), host):
        assert np.array_equal(bits(g), bits(h))
    assert nCT.shape == CT.shape and not nCT[:, K:].any() and not ncn[K:].any()
    ip, ix, v = csr
    row = np.repeat(np.arange(140), np.diff(ip))
    worst = 0.0
    for c in range(K):
        col = nCT[:, c]
        if cnt[c] == 0:
            assert np.array_equal(bits(col), bits(CT[:, c])) and moved2[c] == 0.0
        elif measure == "euclidean":
            # dyadic weights: w x, the weight sum and S 2^-k are exact, so the center differs from the
            # exact mean by the roundings of its n_cf terms, n_cf 2^-(k+1) / W_c, and one division
            # (2^-53 relative); NumPy's own sum of n_cf terms adds n_cf 2^-53 sum |terms| / W_c
            W = w[assign == c].sum()
            assert W == math.ldexp(float(Wq[c]), -KW_E)
            sel = assign[row] == c
            terms = w[row[sel]] * v[sel]
            ref = np.bincount(ix[sel], weights=terms, minlength=F) / W
            n_cf = np.bincount(ix[sel], minlength=F)
            mag = np.bincount(ix[sel], weights=np.abs(terms), minlength=F)
            bound = n_cf * 2.0 ** -(K_E + 1) / W + (n_cf + 1) * 2.0 ** -53 * mag / W
            assert np.all(np.abs(col - ref) <= bound)
            worst = max(worst, float((np.abs(col - ref) / np.where(bound > 0, bound, 1.0)).max()))
        else:
            assert abs(math.sqrt(math.fsum(col * col)) - 1.0) <= 4 * 2.0 ** -53
        # the sums over the features: any order of F terms stays within F 2^-53 sum |terms| of the exact sum
        sq, mv = col * col, (col - CT[:, c]) ** 2
        assert abs(ncn[c] - math.fsum(sq)) <= F * 2.0 ** -53 * math.fsum(sq)
        assert abs(moved2[c] - math.fsum(mv)) <= F * 2.0 ** -53 * math.fsum(mv)
    print(f"K={K} {measure}: max |center - numpy| / bound = {worst:.3e}")


def test_centers_sum_in_the_documented_order():
    _, _, CT, _, (nCT, ncn, moved2) = centers_case(9, "euclidean", "cpu")

    def strided(t):
        s = np.array([math.nan] * 256)
        for lane in range(256):
            acc = 0.0
            for x in t[lane::256]:
                acc = acc + x
            s[lane] = acc
        while s.size > 1:
            s = s[:s.size // 2] + s[s.size // 2:]
        return s[0]

    for c in range(9):
        assert bits(ncn[c]) == bits(strided(nCT[:, c] * nCT[:, c]))
        d = nCT[:, c] - CT[:, c]
        assert bits(moved2[c]) == bits(strided(d * d))


# ---------------------------------------------------------------------------------------------- 5. bad input
@pytest.mark.parametrize("dev", DEVICES)
def test_bad_input_raises_before_any_model(dev):
    csr, w = corpus(140, "float64", True, cosine=True)
    ip, ix, v = csr

    def fit(idx=ix, val=v, weights=w, measure="euclidean"):
        return KM.fit_kmeans(to_vc((ip, idx, val), dev), 3, weights=weights, distance_measure=measure, device=dev,
                             max_iter=2)

    def changed(a, i, x):
        b = a.copy()
        b[i] = x
        return b

    assert fit()["k"] == 3
    for bad in (F, -1, 2 ** 31 - 1):
        with pytest.raises(ValueError):
            fit(idx=changed(ix, 200, bad))
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            fit(val=changed(v, 200, bad))
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            fit(weights=changed(w, 40, bad))
    zero_row = v.copy()
    zero_row[ip[7]:ip[8]] = 0.0
    with pytest.raises(ValueError):
        fit(val=zero_row, measure="cosine")
    assert fit(val=zero_row)["k"] == 3                     # a zero row is a point like any other under euclidean
    # the ops themselves: a flagged row adds nothing and is assigned -1
    CT, cn = centers(9)
    vc = to_vc((ip, changed(ix, int(ip[5]), F + 7), v), dev)
    blk = sparse.km_step(vc, torch.from_numpy(CT).to(dev), torch.from_numpy(cn).to(dev), 9, "euclidean", K_E, KW_E,
                         KC_E, want_rows=True, check=False)
    assert blk.flag == 1 and int(blk.assign[5]) == -1 and int(blk.cnt.sum()) == 139
    with pytest.raises(ValueError):
        sparse.km_step(vc, torch.from_numpy(CT).to(dev), torch.from_numpy(cn).to(dev), 9, "euclidean", K_E, KW_E, KC_E)
    if dev != "cpu":
        torch.cuda.synchronize()                           # the device run ends clean


@pytest.mark.parametrize("dev", DEVICES)
def test_arguments_are_checked_before_any_launch(dev):
    csr, w = corpus(11, "float64", False)
    vc = to_vc(csr, dev)
    CT, cn = (torch.from_numpy(a).to(dev) for a in centers(9))
    for K in (1, 65, 0):
        with pytest.raises(ValueError):
            sparse.km_step(vc, CT, cn, K, "euclidean", K_E, KW_E, KC_E)
        with pytest.raises(ValueError):
            sparse.km_centers(torch.zeros(9 * F, dtype=torch.int64, device=dev),
                              torch.zeros(9, dtype=torch.int64, device=dev), CT, K, K_E, KW_E, "euclidean")
    with pytest.raises(ValueError):
        sparse.km_step(vc, CT, cn, 9, "manhattan", K_E, KW_E, KC_E)
    with pytest.raises(ValueError):
        sparse.km_step(vc, CT[:, :8].contiguous(), cn, 9, "euclidean", K_E, KW_E, KC_E)
    with pytest.raises(ValueError):
        sparse.km_step(vc, CT, cn[:8].contiguous(), 9, "euclidean", K_E, KW_E, KC_E)
    with pytest.raises(ValueError):
        sparse.km_step(vc, CT, cn, 9, "euclidean", K_E, KW_E, 41)
    with pytest.raises(ValueError):
        sparse.km_centers(torch.zeros(8 * F, dtype=torch.int64, device=dev),
                          torch.zeros(9, dtype=torch.int64, device=dev), CT, 9, K_E, KW_E, "euclidean")
    with pytest.raises(ValueError):
        sparse.km_centers(torch.zeros(9 * F, dtype=torch.int64, device=dev),
                          torch.zeros(9, dtype=torch.int64, device=dev), CT, 9, K_E, KW_E, "chebyshev")
    for bad in ({"k": 1}, {"k": 65}, {"k": 3, "init_mode": "kmeans++"}, {"k": 3, "distance_measure": "l1"}):
        with pytest.raises(ValueError):
            KM.fit_kmeans(vc, device=dev, **bad)


# ---------------------------------------------------------------------------------------------- 6. fit
BLOBS, PER, SUPPORT = 3, 20, 12
RANDOM_SEED = 12                                          # its three smallest priorities fall into three blobs


@functools.lru_cache(maxsize=None)
def blobs(dtype_name="float64"):
    """BLOBS x PER rows, blob by blob: blob b holds SUPPORT features of its own with values 10 +- 0.1."""
    rng = np.random.default_rng(21)
    n = BLOBS * PER
    indptr = np.arange(n + 1, dtype=np.int64) * SUPPORT
    support = rng.permutation(F)[:BLOBS * SUPPORT].reshape(BLOBS, SUPPORT)
    label = np.repeat(np.arange(BLOBS), PER)
    idx = np.concatenate([np.sort(support[b]) for b in label]).astype(np.int32)
    val = (10.0 + rng.uniform(-0.1, 0.1, n * SUPPORT)).astype(np.dtype(dtype_name))
    return (indptr, idx, val), label


def dense(csr) -> np.ndarray:
    ip, ix, v = csr
    X = np.zeros((len(ip) - 1, F))
    X[np.repeat(np.arange(len(ip) - 1), np.diff(ip)), ix] = v
    return X


def test_blobs_are_well_separated():
    csr, label = blobs()
    X = dense(csr)
    mean = np.stack([X[label == b].mean(0) for b in range(BLOBS)])
    radius = max(np.linalg.norm(X[label == b] - mean[b], axis=1).max() for b in range(BLOBS))
    gap = min(np.linalg.norm(mean[a] - mean[b]) for a in range(BLOBS) for b in range(a))
    assert gap > 10 * radius
    # the random init of RANDOM_SEED draws one row of every blob (the precondition of its recovery:
    # Lloyd's iteration does not leave a start with two centers in one blob)
    res = fitted("random", "euclidean", "cpu")
    first = {int(np.argmin(((mean - c) ** 2).sum(1))) for c in res["init_centers"]}
    assert first == set(range(BLOBS))


@functools.lru_cache(maxsize=None)
def fitted(init_mode, measure, dev, seed=RANDOM_SEED):
    return KM.fit_kmeans(to_vc(blobs()[0], dev), BLOBS, init_mode=init_mode, distance_measure=measure, seed=seed,
                         device=dev)


def numpy_lloyd(X, C, max_iter=20, tol=1e-4):
    """Lloyd's iteration in NumPy from the centers C: (centers, iterations), Spark's stopping rule."""
    for it in range(1, max_iter + 1):
        a = np.argmin(((X[:, None, :] - C[None]) ** 2).sum(2), axis=1)
        new = np.stack([X[a == c].mean(0) if np.any(a == c) else C[c] for c in range(len(C))])
        moved = ((new - C) ** 2).sum(1)
        C = new
        if np.all(moved <= tol * tol):
            return C, it
    return C, max_iter


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("init_mode", ["random", "k-means||"])
def test_fit_recovers_the_blobs_and_equals_numpy_lloyd(init_mode, measure, dev):
    csr, label = blobs()
    res = fitted(init_mode, measure, dev)
    assert res["k"] == BLOBS and res["centers"].shape == (BLOBS, F) and res["num_iter"] >= 1
    pred = KM.predict_kmeans(to_vc(csr, dev), res["centers"], measure).cpu().numpy()
    assert len(set(zip(label.tolist(), pred.tolist()))) == BLOBS and len(set(pred.tolist())) == BLOBS
    assert sorted(res["sizes"].tolist()) == [PER] * BLOBS
    host = fitted(init_mode, measure, "cpu")
    assert np.array_equal(bits(res["centers"]), bits(host["centers"]))
    assert (res["costq"], res["num_iter"], res["ek"]) == (host["costq"], host["num_iter"], host["ek"])
    assert bits(res["cost"]) == bits(host["cost"]) and res["cost"] > 0
    if measure == "euclidean":
        X = dense(csr)
        ref, iters = numpy_lloyd(X, res["init_centers"])
        assert iters == res["num_iter"]
        # unit weights: a center is the exact mean of its PER rows up to PER roundings of 2^-(k+1), one
        # division and NumPy's own sum of PER terms
        bound = PER * 2.0 ** -(res["ek"] + 1) / PER + (PER + 1) * 2.0 ** -53 * np.abs(X).max(0)
        assert np.all(np.abs(res["centers"] - ref) <= bound[None, :])
    else:
        assert np.all(np.abs(np.sqrt((res["centers"] ** 2).sum(1)) - 1.0) <= 4 * 2.0 ** -53)


def test_a_fit_is_a_function_of_the_seed():
    csr, _ = blobs()
    vc = to_vc(csr, "cpu")
    for mode in ("random", "k-means||"):
        a = KM.fit_kmeans(vc, BLOBS, init_mode=mode, seed=RANDOM_SEED, device="cpu")
        b = fitted(mode, "euclidean", "cpu")
        assert np.array_equal(bits(a["centers"]), bits(b["centers"])) and a["costq"] == b["costq"]
        assert np.array_equal(bits(a["init_centers"]), bits(b["init_centers"]))
    other = KM.fit_kmeans(vc, BLOBS, init_mode="random", seed=RANDOM_SEED + 1, device="cpu")
    assert not np.array_equal(bits(other["init_centers"]), bits(fitted("random", "euclidean", "cpu")["init_centers"]))


def test_fewer_distinct_rows_than_k_give_fewer_centers():
    ip = np.arange(7, dtype=np.int64) * 2
    ix = np.tile(np.array([3, 9], dtype=np.int32), 6)
    v = np.concatenate([[1.0, 2.0]] * 3 + [[5.0, 1.0]] * 3)
    res = KM.fit_kmeans(to_vc((ip, ix, v), "cpu"), 4, device="cpu", seed=1)
    assert res["k"] == 2 and sorted(res["sizes"].tolist()) == [3, 3] and res["cost"] == 0.0
    same_rows = (ip, ix, np.tile([1.0, 2.0], 6))
    with pytest.raises(ValueError):
        KM.fit_kmeans(to_vc(same_rows, "cpu"), 4, device="cpu", seed=1)


def test_more_candidates_than_max_k_fold_by_the_minimum():
    """k-means|| with k = 64 oversamples to more than 64 candidates: the passes are chunked."""
    rng = np.random.default_rng(2)
    n = 600
    ip = np.arange(n + 1, dtype=np.int64) * 4
    ix = np.concatenate([np.sort(rng.choice(F, 4, replace=False)) for _ in range(n)]).astype(np.int32)
    v = rng.uniform(0.5, 2.0, 4 * n)
    res = KM.fit_kmeans(to_vc((ip, ix, v), "cpu"), 64, device="cpu", seed=4, max_iter=3, init_steps=3)
    assert res["k"] == 64 and int(res["sizes"].sum()) == n and res["num_iter"] == 3


# ---------------------------------------------------------------------------------------------- 7. data parallel
def _dp_weights():
    w = np.random.default_rng(8).uniform(0.5, 1.5, BLOBS * PER)
    w[-2] = 3.25                                          # only the last shard holds the largest weight
    return w


DP_CASES = (("random", "euclidean"), ("k-means||", "euclidean"), ("k-means||", "cosine"))


def _dp_result(res):
    return res["centers"].tobytes(), res["costq"], res["num_iter"], res["sizes"].tolist(), res["ek"], res["ekw"]


def _dp_fit(rank, world):
    """Every case in one process group: a spawn costs more than the fits."""
    from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

    (ip, ix, v), _ = blobs("float32")
    w = _dp_weights()
    lo, hi = shard_range(len(w), rank, world)
    shard = (ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]], v[ip[lo]:ip[hi]])
    return [_dp_result(KM.fit_kmeans(to_vc(shard, "cpu"), BLOBS, weights=w[lo:hi], init_mode=init_mode,
                                     distance_measure=measure, seed=RANDOM_SEED, device="cpu"))
            for init_mode, measure in DP_CASES]


@pytest.mark.parametrize("world", [2, 3])
def test_data_parallel_fit_equals_single_process(world):
    from fraud_detection_spark_kafka_llm_amd.parallel.launch import spawn

    csr, label = blobs("float32")
    if world == 3:                                        # every shard holds all rows of one blob
        from fraud_detection_spark_kafka_llm_amd.parallel.dist import shard_range

        assert all(set(label[slice(*shard_range(len(label), r, 3))]) == {r} for r in range(3))
    outs = spawn(_dp_fit, world, backend="gloo")
    assert all(o == outs[0] for o in outs)
    for (init_mode, measure), got in zip(DP_CASES, outs[0]):
        single = KM.fit_kmeans(to_vc(csr, "cpu"), BLOBS, weights=_dp_weights(), init_mode=init_mode,
                               distance_measure=measure, seed=RANDOM_SEED, device="cpu")
        assert got == _dp_result(single), (init_mode, measure)
        assert single["k"] == BLOBS and sorted(single["sizes"].tolist()) == [PER] * BLOBS


# ---------------------------------------------------------------------------------------------- 8. API
def test_defaults_are_sparks():
    from fraud_detection_spark_kafka_llm_amd.ml import KMeans

    km = KMeans()
    assert (km.getK(), km.getMaxIter(), km.getTol(), km.getInitMode(), km.getInitSteps(), km.getDistanceMeasure()) == \
        (2, 20, 1e-4, "k-means||", 2, "euclidean")
    assert (km.getFeaturesCol(), km.getPredictionCol()) == ("features", "prediction") and not km.isSet("weightCol")
    assert isinstance(km.getSeed(), int)


@functools.lru_cache(maxsize=None)
def blob_model(measure="euclidean"):
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, KMeans

    csr, label = blobs()
    df = Frame({"features": to_vc(csr, "cpu"), "w": np.ones(len(label))})
    return KMeans(k=BLOBS, seed=RANDOM_SEED, distanceMeasure=measure, weightCol="w").fit(df), df


def test_model_transform_predict_and_summary():
    from fraud_detection_spark_kafka_llm_amd.ml.linalg import SparseVector

    model, df = blob_model()
    csr, label = blobs()
    out = model.transform(df)
    pred = out.column("prediction")
    pred = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
    assert pred.dtype == np.int32 and len(set(zip(label.tolist(), pred.tolist()))) == BLOBS
    cs = model.clusterCenters()
    assert len(cs) == BLOBS and all(isinstance(c, np.ndarray) and c.shape == (F,) for c in cs) and model.numFeatures == F
    ref = fitted("k-means||", "euclidean", "cpu")
    assert np.array_equal(bits(np.stack(cs)), bits(ref["centers"]))
    ip, ix, v = csr
    for r in (0, PER, 2 * PER + 3):
        assert model.predict(SparseVector(F, ix[ip[r]:ip[r + 1]], v[ip[r]:ip[r + 1]])) == pred[r]
    s = model.summary
    assert model.hasSummary and s.k == BLOBS and sorted(s.clusterSizes) == [PER] * BLOBS and s.numIter == ref["num_iter"]
    assert s.trainingCost == ref["cost"] > 0
    assert set(np.unique(blob_model("cosine")[0].transform(df).column("prediction").cpu().numpy())) == {0, 1, 2}


def test_spark_layout_round_trip_is_bitwise(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.io import spark_format as sf
    from fraud_detection_spark_kafka_llm_amd.ml import KMeansModel

    model, df = blob_model("cosine")
    path = tmp_path / "kmeans"
    model.save(str(path))
    assert sf.verify_tree(path) == []
    assert sf.read_metadata(path)["class"] == "org.apache.spark.ml.clustering.KMeansModel"
    schema = sf.spark_schema_of(path)
    assert [(f["name"], f["type"] if isinstance(f["type"], str) else f["type"]["type"]) for f in schema["fields"]] == \
        [("clusterIdx", "integer"), ("clusterCenter", "udt")]
    assert schema["fields"][1]["type"]["class"] == "org.apache.spark.ml.linalg.VectorUDT"
    rows = sf.read_data_parquet(path).to_pylist()
    assert [r["clusterIdx"] for r in rows] == list(range(BLOBS)) and all(r["clusterCenter"]["type"] == 1 for r in rows)
    back = KMeansModel.load(str(path))
    assert isinstance(back, KMeansModel) and back.getDistanceMeasure() == "cosine" and back.getK() == BLOBS
    assert np.array_equal(bits(back.centers), bits(model.centers)) and not back.hasSummary
    a, b = (m.transform(df).column("prediction").cpu().numpy() for m in (model, back))
    assert np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def dialogues():
    from fraud_detection_spark_kafka_llm_amd.data import synth
    from fraud_detection_spark_kafka_llm_amd.ml import Frame, TextColumn

    pt, y = synth.generate(synth.SynthConfig(n=300, seed=31))
    raw = TextColumn(pt.strings())
    return Frame({"dialogue": raw, "clean_text": TextColumn.cleaned_from(raw), "labels": y.numpy()})


def test_pipeline_fits_transforms_and_does_not_compile(tmp_path):
    from fraud_detection_spark_kafka_llm_amd.ml import (IDF, HashingTF, KMeans, KMeansModel, Pipeline, PipelineModel,
                                                      StopWordsRemover, Tokenizer)

    df = dialogues()
    stages = [Tokenizer(inputCol="clean_text", outputCol="words"),
              StopWordsRemover(inputCol="words", outputCol="filtered_words"),
              HashingTF(inputCol="filtered_words", outputCol="raw_features", numFeatures=4096),
              IDF(inputCol="raw_features", outputCol="features"), KMeans(k=3, seed=7, maxIter=5)]
    model = Pipeline(stages=stages).fit(df)
    km = model.stages[-1]
    assert isinstance(km, KMeansModel) and km.numFeatures == 4096 and km.summary.k == 3
    out = model.transform(df)
    pred = out.column("prediction").cpu().numpy()
    assert pred.shape == (len(df),) and pred.dtype == np.int32 and np.array_equal(np.bincount(pred, minlength=3),
                                                                                  km.summary.clusterSizes)
    staged = df
    for s in model.stages:
        staged = s.transform(staged)
    assert np.array_equal(staged.column("prediction").cpu().numpy(), pred)
    with pytest.raises(NotImplementedError, match="assign tail"):
        model.compile()
    model.save(str(tmp_path / "p"))
    back = PipelineModel.load(str(tmp_path / "p"))
    assert np.array_equal(back.transform(df).column("prediction").cpu().numpy(), pred)


def test_train_cli_adds_kmeans_on_request(tmp_path):
    from fraud_detection_spark_kafka_llm_amd import train
    from fraud_detection_spark_kafka_llm_amd.ml import KMeansModel

    common = ["--data", "", "--synthetic", "300", "--no-plots", "--num-trees", "2", "--max-depth", "2",
              "--out-dir", str(tmp_path), "--device", "cpu"]
    summary = train.main(common + ["--kmeans", "3"])
    km = summary["KMeans"]
    assert km["k"] == 3 and sum(km["clusterSizes"]) > 0 and len(km["scamShare"]) == 3
    assert all(0.0 <= s <= 1.0 for s in km["scamShare"])
    back = KMeansModel.load(str(tmp_path / "kmeans_model"))
    assert len(back.clusterCenters()) == 3


# ---------------------------------------------------------------------------------------------- 9. self-test
def test_km_selftest_runs_clean_under_sanitizers():
    res = subprocess.run([sys.executable, "-m", "fraud_detection_spark_kafka_llm_amd._build", "--km-selftest"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "km_selftest: ok" in res.stdout
