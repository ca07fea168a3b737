"""The row and node kernels that run around the histogram at every tree level (csrc/tree_kernels.hip:
quantisation, slot map, partition, sibling subtraction, best split, gradient and leaf update) and
their host twins (csrc/tree_cpu.cpp), each against a reference written here from the documented
contract: numpy fp64 where every operation is exact, Python ints otherwise, ``np.longdouble`` for
``exp``. The twins share csrc/tree.h, so "device == host" alone cannot see a wrong exponent, tie
rule or digit; the references below share nothing with either.

Every test runs on the host twin; its ``cuda:0`` case runs the kernel against the same reference
and, where the contract is bitwise, against the host twin's bytes. Output buffers are pre-filled
with a sentinel, and where the contract says "untouched" the sentinel must have survived."""
import functools
import math

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.models.rf_sampling import hash_uniform
from fraud_detection_spark_kafka_llm_amd.ops import native

GPU = "cuda:0"
DEVS = ["cpu", pytest.param(GPU, marks=pytest.mark.gpu)]
S32 = -1431655766          # 0xAAAAAAAA as int32: the int32 sentinel
S8 = 0xA5


def _t(a, dev):
    """numpy array (or None) -> tensor on dev; the device copy never aliases the shared input"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.clone() if dev == "cpu" else t.to(dev)


def _np(t):
    return t.cpu().numpy()


def _check(dev, run, verify):
    """run(dev) -> {name: array}; verify(out) asserts it against the reference; on the GPU the
    host twin's outputs must also be the same bytes."""
    out = run(dev)
    verify(out)
    if dev != "cpu":
        host = run("cpu")
        for k, v in out.items():
            assert v.tobytes() == host[k].tobytes(), f"{k}: device bytes differ from the host twin's"


# ----------------------------------------------------------------------------------- quantisation
def _digits4(q):
    """balanced base-256 digits of q (int64 array) as uint32 words, byte i = d_i & 0xff"""
    rest = q.astype(np.int64).copy()
    word = np.zeros(q.shape, np.uint32)
    back = np.zeros(q.shape, np.int64)
    for i in range(4):
        d = (rest + 128) % 256 - 128
        rest = (rest - d) // 256
        byte = d & 0xFF
        word |= byte.astype(np.uint32) << np.uint32(8 * i)
        back += np.where(byte >= 128, byte - 256, byte) * 256 ** i
    assert (rest == 0).all(), "q has more than 4 balanced digits"
    assert (back == q).all()
    return word


def _digits1(q):
    return (q.astype(np.int64) & 0xFF).astype(np.uint32)


def _poisson1(u):
    """Poisson(1) by CDF inversion: the loop documented at poisson1 in csrc/tree.h"""
    p = 0.36787944117144233
    cdf, k = p, 0
    while u > cdf and k < 32:
        k += 1
        p /= k
        cdf += p
    return k


def _stats(c):
    """the two fp64 row statistics of a quantisation case (every product exact in fp64)"""
    if c["mode"] == 0:
        w = c["w"].astype(np.float64) if c["w"] is not None else 1.0
        return c["g"].astype(np.float64) * w, c["h"].astype(np.float64) * w
    y = c["label"].astype(np.float64)
    w = c["w"].astype(np.float64) if c["w"] is not None else np.ones(len(y))
    if c["boot"]:
        rows = torch.arange(c["row0"], c["row0"] + len(y), dtype=torch.int64)
        u = hash_uniform(c["seed"], c["tree"], rows).numpy()
        w = w * np.array([_poisson1(float(x)) for x in u], np.float64)
    return w * (1.0 - y), w * y


def _quant_ref(c):
    v = _stats(c)
    m = [float(np.max(np.abs(x))) if x.size else 0.0 for x in v]
    k = [0, 0]
    if c["use_max"]:
        k = [0 if mm == 0.0 else 30 - math.frexp(mm)[1] for mm in m]
    q = []
    for x, kk in zip(v, k):
        s = np.rint(np.ldexp(x, kk))                     # exact scaling, ties to even
        assert np.isfinite(s).all() and (np.abs(s) <= 2.0 ** 30).all()
        q.append(s.astype(np.int64))
    dig = _digits4 if c["np"] == 4 else _digits1
    return dict(m=np.array(m), k=k, q=q, totals=[sum(x.tolist()) for x in q],
                rowdig=np.stack([dig(q[0]), dig(q[1])], 1))


def _quant_run(c, dev, pad=37):
    C = native.lib()
    N = len(c["g"] if c["mode"] == 0 else c["label"])
    G, H, L, W = (_t(c.get(x), dev) for x in ("g", "h", "label", "w"))
    seed, tree, boot, row0 = c.get("seed", 0), c.get("tree", 0), c.get("boot", False), c.get("row0", 0)
    out, mx = {}, None
    if c["use_max"]:
        mx = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
        C.tree_quant_max(G, H, L, W, seed, tree, boot, c["mode"], N, mx, row0)
        out["max"] = _np(mx)
    rowdig = torch.full((N, 2), S32, dtype=torch.int32, device=dev)
    kexp = torch.full((2,), -99, dtype=torch.int32, device=dev)
    totals = torch.full((2,), -99, dtype=torch.int64, device=dev)
    digp = torch.full((2 * c["np"], N + pad), S8, dtype=torch.uint8, device=dev)
    C.tree_quant(G, H, L, W, seed, tree, boot, c["mode"], c["np"], mx, rowdig, kexp, totals, digp, row0)
    out.update(kexp=_np(kexp), totals=_np(totals), rowdig=_np(rowdig).view(np.uint32), digp=_np(digp))
    return out


def _quant_verify(c, ref, out):
    N, npl = len(ref["rowdig"]), c["np"]
    if c["use_max"]:
        assert out["max"].view(np.uint64).tolist() == ref["m"].view(np.uint64).tolist()
    assert out["kexp"].tolist() == ref["k"]
    assert out["totals"].tolist() == ref["totals"]
    bad = np.flatnonzero((out["rowdig"] != ref["rowdig"]).any(1))
    assert bad.size == 0, (bad[:5], out["rowdig"][bad[:5]], ref["rowdig"][bad[:5]])
    for s in range(2):
        for p in range(npl):
            plane = (ref["rowdig"][:, s] >> np.uint32(8 * p)) & 0xFF
            assert np.array_equal(out["digp"][s * npl + p, :N], plane), (s, p)
    assert (out["digp"][:, N:] == S8).all(), "digp columns past N were written"


def _quant_case(g=None, h=None, w=None, label=None, mode=0, npl=4, use_max=True, **kw):
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)
    return dict(g=f32(g), h=f32(h), w=f32(w), label=f32(label), mode=mode, np=npl, use_max=use_max,
                seed=kw.get("seed", 0), tree=kw.get("tree", 0), boot=kw.get("boot", False), row0=kw.get("row0", 0))


@functools.lru_cache(maxsize=None)
def _quant_rows(N, weighted):
    rng = np.random.default_rng(N)
    c = _quant_case(rng.standard_normal(N), rng.random(N) * 0.25, rng.random(N) * 2 if weighted else None)
    return c, _quant_ref(c)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_quant_block_and_prologue_step_edges(N, weighted, dev):
    c, ref = _quant_rows(N, weighted)
    _check(dev, lambda d: _quant_run(c, d), lambda o: _quant_verify(c, ref, o))


TIE_J = [0, 1, 2, 3, -1, -2, -3, -4]
CARRY_Q = [127, 128, -128, -129, 0x7F80, 0x8080, -0x8081, 2 ** 29, -2 ** 29, 2 ** 29 - 1]


def _edge_cases():
    one_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    tiny = np.float32(2.0 ** -149)
    h = [0.125, 0.0625, 0.03125]
    out = {
        "max 1.0": _quant_case([1.0, 0.3, -0.7], h),
        "max 0.25": _quant_case([0.1, 0.25, -0.2], h),
        "max just below 1.0": _quant_case([0.5, -0.25, one_below], h),
        "all zero": _quant_case([0.0, -0.0, 0.0], [0.0, 0.0, 0.0]),
        "smallest denormal": _quant_case([tiny, 0.0, -tiny], h),
        "negative maximum": _quant_case([0.5, -0.75, 0.25], h),
        "second statistic": _quant_case(h, [1.0, -0.25, one_below]),
        "ties": _quant_case([1.0] + [(j + 0.5) * 2.0 ** -29 for j in TIE_J], [0.5] * 9),
    }
    # q / 2^29 as g * w, both float32: 2^29 - 1 = 256999 * 2089 needs the product, the others fit g
    g = [1.0] + [q / 2.0 ** 29 for q in CARRY_Q[:-1]] + [256999 / 2.0 ** 18]
    w = [1.0] * len(CARRY_Q) + [2089 / 2.0 ** 11]
    out["digit carries"] = _quant_case(g, [0.5] * len(g), w)
    return out


EDGES = _edge_cases()


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("name", list(EDGES))
def test_quant_exponent_rounding_and_digit_edges(name, dev):
    c = EDGES[name]
    ref = _quant_ref(c)
    # the reference itself, against the values the contract spells out
    expect_k = {"max 1.0": 29, "max 0.25": 31, "max just below 1.0": 30, "all zero": 0, "smallest denormal": 178,
                "negative maximum": 30}
    if name in expect_k:
        assert ref["k"][0] == expect_k[name]
    if name in ("max 1.0", "max 0.25", "smallest denormal"):
        assert max(abs(x) for x in ref["q"][0].tolist()) == 2 ** 29
    if name == "all zero":
        assert ref["k"] == [0, 0] and not ref["rowdig"].any()
    if name == "ties":
        assert ref["k"][0] == 29 and ref["q"][0].tolist() == [2 ** 29, 0, 2, 2, 4, 0, -2, -2, -4]
    if name == "digit carries":
        assert ref["k"][0] == 29 and ref["q"][0].tolist() == [2 ** 29] + CARRY_Q
        assert [hex(x) for x in ref["rowdig"][1:5, 0].tolist()] == ["0x7f", "0x180", "0x80", "0xff7f"]
    _check(dev, lambda d: _quant_run(c, d), lambda o: _quant_verify(c, ref, o))


@functools.lru_cache(maxsize=None)
def _quant_max_strided():
    N = 2048 * 256 + 257                       # rows past 2048 * 256 belong to the strided iteration
    rng = np.random.default_rng(5)
    g, h = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    g[-1], h[2048 * 256] = -9.5, 11.25
    c = _quant_case(g, h)
    return c, np.array([9.5, 11.25])


@pytest.mark.parametrize("dev", DEVS)
def test_quant_max_grid_stride(dev):
    c, m = _quant_max_strided()
    assert np.abs(c["g"][:-1]).max() < 9.5 and np.abs(np.delete(c["h"], 2048 * 256)).max() < 11.25
    C = native.lib()
    mx = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    C.tree_quant_max(_t(c["g"], dev), _t(c["h"], dev), None, None, 0, 0, False, 0, len(c["g"]), mx, 0)
    assert _np(mx).view(np.uint64).tolist() == m.view(np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def _quant_strided():
    N = 2048 * 1024 + 1027                     # rows past 2048 * 1024 belong to the strided iteration
    rng = np.random.default_rng(6)
    c = _quant_case(rng.standard_normal(N), rng.random(N), rng.random(N) + 0.5)
    assert np.count_nonzero(c["g"][2048 * 1024:]) > 1000
    return c, _quant_ref(c)


@pytest.mark.parametrize("dev", DEVS)
def test_quant_grid_stride(dev):
    c, ref = _quant_strided()

    def verify(o):
        assert o["kexp"].tolist() == ref["k"] and o["totals"].tolist() == ref["totals"]
        assert np.array_equal(o["rowdig"][-2000:], ref["rowdig"][-2000:])
        _quant_verify(c, ref, o)

    _check(dev, lambda d: _quant_run(c, d), verify)


@functools.lru_cache(maxsize=None)
def _count_case(kind):
    N = 4099
    rng = np.random.default_rng(8)
    label = (rng.random(N) < 0.4)
    if kind == "np1":
        c = _quant_case(label=label, w=rng.integers(0, 4, N), mode=1, npl=1, use_max=False)
    elif kind == "np1 unweighted":
        c = _quant_case(label=label, mode=1, npl=1, use_max=False)
    elif kind == "np4":
        c = _quant_case(label=label, w=rng.random(N) * 3, mode=1, npl=4)
    elif kind == "np1 bootstrap":
        c = _quant_case(label=label, w=rng.integers(0, 4, N), mode=1, npl=1, use_max=False, boot=True, seed=12345,
                        tree=7, row0=1000003)
    else:
        c = _quant_case(label=label, w=rng.random(N) * 3, mode=1, npl=4, boot=True, seed=99, tree=3, row0=777)
    return c, _quant_ref(c)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("kind", ["np1", "np1 unweighted", "np4", "np1 bootstrap", "np4 bootstrap"])
def test_quant_class_counts(kind, dev):
    c, ref = _count_case(kind)
    if c["boot"]:                              # the draws are not all 0 or 1, and fit np = 1's byte
        v0, v1 = _stats(c)
        assert (v0 + v1).max() >= 4 and (c["np"] == 4 or (v0 + v1).max() <= 127)
    _check(dev, lambda d: _quant_run(c, d), lambda o: _quant_verify(c, ref, o))


# --------------------------------------------------------------------------------------- slot map
@functools.lru_cache(maxsize=None)
def _slot_case(N, slot_base, nslots):
    rng = np.random.default_rng(N + 7 * slot_base + nslots)
    nn = 300
    node_slot = rng.integers(-1, slot_base + nslots + 12, nn).astype(np.int32)
    node_slot[:4] = [-1, slot_base, slot_base + nslots, slot_base + nslots - 1]
    row_node = rng.integers(0, nn, N).astype(np.int32)
    for i, v in enumerate([-1, nn, nn + 5, 0, 1, 2, 3]):
        if N > 7 * i + 3:
            row_node[7 * i + 3] = v
    rowdig = rng.integers(-2 ** 31, 2 ** 31, (N, 2)).astype(np.int32)
    return row_node, node_slot, rowdig


def _slot_ref(row_node, node_slot, slot_base, nslots):
    nn = len(node_slot)
    ok = (row_node >= 0) & (row_node < nn)
    s = np.where(ok, node_slot[np.clip(row_node, 0, nn - 1)].astype(np.int64) - slot_base, -1)
    return s, np.where((s >= 0) & (s < nslots), s, 0xFF).astype(np.uint8)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("nslots", [1, 64, 255])
@pytest.mark.parametrize("slot_base", [0, 3])
@pytest.mark.parametrize("N", [1, 255, 257, 4099])
def test_slot8_masked_and_pack(N, slot_base, nslots, dev):
    row_node, node_slot, rowdig = _slot_case(N, slot_base, nslots)
    s, slot8 = _slot_ref(row_node, node_slot, slot_base, nslots)
    masked = np.where((s == 0)[:, None], rowdig, 0).astype(np.int32)
    s0, slot0 = _slot_ref(row_node, node_slot, 0, nslots)
    d = rowdig.view(np.uint32)
    pack = slot0.astype(np.uint32) | ((d[:, 0] & 0xFF) << np.uint32(8)) | ((d[:, 1] & 0xFF) << np.uint32(16))
    if N == 4099:
        assert {0xFF, 0}.issubset(set(slot8.tolist())) and (masked != 0).any()

    def run(dv):
        C = native.lib()
        rn, ns, rd = _t(row_node, dv), _t(node_slot, dv), _t(rowdig, dv)
        out = {}
        o = torch.full((N,), S8, dtype=torch.uint8, device=dv)
        C.tree_slot8(rn, ns, slot_base, nslots, o, None, None)
        out["slot8"] = _np(o)
        if nslots == 1:
            o = torch.full((N,), S8, dtype=torch.uint8, device=dv)
            mk = torch.full((N, 2), S32, dtype=torch.int32, device=dv)
            C.tree_slot8(rn, ns, slot_base, 1, o, rd, mk)
            out["slot8_m"], out["masked"] = _np(o), _np(mk)
        if slot_base == 0:
            pk = torch.full((N,), S32, dtype=torch.int32, device=dv)
            C.tree_slot_pack(rn, ns, nslots, rd, pk)
            out["pack"] = _np(pk).view(np.uint32)
        assert np.array_equal(_np(rn), row_node) and np.array_equal(_np(rd), rowdig)
        return out

    def verify(o):
        assert np.array_equal(o["slot8"], slot8)
        if nslots == 1:
            assert np.array_equal(o["slot8_m"], slot8) and np.array_equal(o["masked"], masked)
        if slot_base == 0:
            assert np.array_equal(o["pack"], pack)

    _check(dev, run, verify)


@functools.lru_cache(maxsize=None)
def _big_rows():
    """(row_node, node table values) at the 8192-block grid cap of the one-row-per-thread passes"""
    N = 8192 * 256 + 3
    rng = np.random.default_rng(9)
    return rng.integers(0, 300, N).astype(np.int32), rng.standard_normal(N), rng.standard_normal(300)


@pytest.mark.parametrize("dev", DEVS)
def test_slot8_grid_cap(dev):
    row_node = _big_rows()[0]
    N = len(row_node)
    node_slot = _slot_case(4099, 3, 64)[1]
    slot8 = _slot_ref(row_node, node_slot, 3, 64)[1]

    def run(dv):
        o = torch.full((N,), S8, dtype=torch.uint8, device=dv)
        native.lib().tree_slot8(_t(row_node, dv), _t(node_slot, dv), 3, 64, o, None, None)
        return dict(slot8=_np(o))

    _check(dev, run, lambda o: np.testing.assert_array_equal(o["slot8"], slot8))


# -------------------------------------------------------------------------------------- partition
NN = 48                                        # node table size: nodes 0..9 hold rows, children from 10


@functools.lru_cache(maxsize=None)
def _partition_case(N, dense_on):
    """One level's partition: leaves, column splits (an empty column, a column present in every row,
    thresholds at bin 0 and at the largest bin, both default sides), dense-block splits, rows at
    out-of-range nodes. Child ids are distinct, so no row can be moved twice."""
    rng = np.random.default_rng(3 * N + dense_on)
    F = 10
    dens = np.array([0.0, 1.0, 0.4, 0.5, 0.3, 0.6, 0.5, 0.4, 0.2, 0.7])
    present = rng.random((N, F)) < dens
    bins = rng.integers(0, 9, (N, F)).astype(np.uint8)
    colptr, rows_, bins_ = [0], [], []
    for f in range(F):
        r = np.flatnonzero(present[:, f])
        rows_.append(r)
        bins_.append(bins[r, f])
        colptr.append(colptr[-1] + len(r))
    csc_row = np.concatenate(rows_ + [np.zeros(8, np.int64)]).astype(np.int32)       # (+ readable padding)
    csc_bin = np.concatenate(bins_ + [np.zeros(8, np.uint8)]).astype(np.uint8)
    colptr = np.array(colptr, np.int64)
    row_node = rng.integers(0, 10, N).astype(np.int32)
    for i, v in enumerate([-1, NN, -1, NN + 3]):
        if N > 5 * i + 2:
            row_node[5 * i + 2] = v
    default_child = np.full(NN, -1, np.int32)
    # column splits: (node, feature, threshold bin, left is default)
    top = lambda f: int(bins_[f].max()) if len(bins_[f]) else 0
    cs = [(1, 0, 3, 1), (2, 1, 0, 1), (3, 2, top(2), 0), (4, 3, 4, 1), (5, 3, 2, 0), (6, 5, 0, 0)]
    if not dense_on:
        cs += [(7, 6, 5, 1), (8, 7, top(7), 1)]
    sp = dict(feat=[], dflt=[], other=[], bin=[], lid=[])
    for n, f, thr, lid in cs:
        default_child[n] = 10 + 2 * n
        for k, v in zip(sp, (f, 10 + 2 * n, 11 + 2 * n, thr, lid)):
            sp[k].append(v)
    n_splits = len(cs)
    # entries past the count: they would move node 2's and node 4's rows if they were applied
    for f, dflt, other, thr, lid in [(1, 14, 40, 8, 0), (5, 18, 41, 8, 0), (2, 12, 42, 0, 1)]:
        for k, v in zip(sp, (f, dflt, other, thr, lid)):
            sp[k].append(v)
    sp = {k: np.array(v, np.int32) for k, v in sp.items()}
    node_dense = dense = None
    if dense_on:
        dense = rng.integers(0, 9, (3, N + 19)).astype(np.uint8)
        node_dense = np.tile(np.array([-1, 0, 0, 0], np.int32), (NN, 1))
        for n, (hot, thr) in {7: (2, 3), 8: (0, 0)}.items():
            default_child[n] = 10 + 2 * n
            node_dense[n] = (hot, thr, 10 + 2 * n, 11 + 2 * n)
        node_dense[9] = (1, 3, 44, 45)         # a leaf (default_child = -1): its rows stay
    pack_slot = rng.integers(0, 255, NN).astype(np.int32)
    pack_slot[[12, 15, 24, 27, 0]] = [-1, 255, 300, -1, 254]
    pack_dig = rng.integers(-2 ** 31, 2 ** 31, (N, 2)).astype(np.int32)
    return dict(N=N, colptr=colptr, csc_row=csc_row, csc_bin=csc_bin, row_node=row_node, default_child=default_child,
                sp=sp, n_splits=n_splits, node_dense=node_dense, dense=dense, pack_slot=pack_slot, pack_dig=pack_dig)


def _partition_ref(c):
    rn, N = c["row_node"], c["N"]
    ok = (rn >= 0) & (rn < NN)
    cl = np.clip(rn, 0, NN - 1)
    dc = np.where(ok, c["default_child"][cl], -1)
    new = np.where(dc >= 0, dc, rn)
    if c["node_dense"] is not None:
        nd = c["node_dense"][cl]
        use = (dc >= 0) & (nd[:, 0] >= 0)
        b = c["dense"][np.clip(nd[:, 0], 0, None), np.arange(N)]
        new = np.where(use, np.where(b <= nd[:, 1], nd[:, 2], nd[:, 3]), new)
    new = new.astype(np.int32)
    sp = c["sp"]
    for s in range(c["n_splits"]):
        e0, e1 = c["colptr"][sp["feat"][s]], c["colptr"][sp["feat"][s] + 1]
        rows = c["csc_row"][e0:e1]
        left = c["csc_bin"][e0:e1].astype(np.int32) <= sp["bin"][s]
        mv = (left != bool(sp["lid"][s])) & (new[rows] == sp["dflt"][s])
        new[rows[mv]] = sp["other"][s]
    ps = np.where((new >= 0) & (new < NN), c["pack_slot"][np.clip(new, 0, NN - 1)], -1)
    sb = np.where((ps >= 0) & (ps < 255), ps, 0xFF).astype(np.uint32)
    d = c["pack_dig"].view(np.uint32)
    pack = sb | ((d[:, 0] & 0xFF) << np.uint32(8)) | ((d[:, 1] & 0xFF) << np.uint32(16))
    return new, pack


def _partition_verify(c, new, out):
    rn = c["row_node"]
    assert np.array_equal(out["row_node"], new), np.flatnonzero(out["row_node"] != new)[:8]
    stay = (rn < 0) | (rn >= NN) | (c["default_child"][np.clip(rn, 0, NN - 1)] < 0)
    assert np.array_equal(out["row_node"][stay], rn[stay])
    if c["N"] == 4099:                         # every kind of row is there, and both passes moved rows
        assert stay.any() and (rn >= NN).any() and (rn < 0).any()
        # (node 1 splits on the empty column; node 8's column split keeps every row on the default side)
        assert set(c["sp"]["other"][:c["n_splits"]].tolist()) - {13, 27} <= set(new.tolist())
        assert c["colptr"][2] - c["colptr"][1] > 256 * 4 and c["colptr"][1] == c["colptr"][0]


PART_N = [1, 7, 8, 9, 511, 512, 513, 4099]


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("dense_on", [False, True])
@pytest.mark.parametrize("N", PART_N)
def test_partition_rows_then_items(N, dense_on, dev):
    c = _partition_case(N, dense_on)
    new, _ = _partition_ref(c)
    sp, ns = c["sp"], c["n_splits"]
    start, end, split = [], [], []
    for s in range(ns):                        # the split columns in chunks of up to 300 entries
        e0, e1 = int(c["colptr"][sp["feat"][s]]), int(c["colptr"][sp["feat"][s] + 1])
        for a in range(e0, e1, 300):
            start.append(a)
            end.append(min(a + 300, e1))
            split.append(s)
    items = [np.array(start, np.int64), np.array(end, np.int64), np.array(split, np.int32)]

    def run(dv):
        rn = _t(c["row_node"], dv)
        assert rn.data_ptr() % 16 == 0
        native.lib().tree_partition(rn, _t(c["default_child"], dv), *(_t(x, dv) for x in items),
                                    *(_t(sp[k][:ns], dv) for k in ("dflt", "other", "bin", "lid")),
                                    _t(c["csc_row"], dv), _t(c["csc_bin"], dv), _t(c["node_dense"], dv),
                                    _t(c["dense"], dv))
        return dict(row_node=_np(rn))

    _check(dev, run, lambda o: _partition_verify(c, new, o))


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("with_pack", [False, True])
@pytest.mark.parametrize("wps", [1, 4])
@pytest.mark.parametrize("dense_on", [False, True])
@pytest.mark.parametrize("N", PART_N)
def test_partition_cols_counted_splits_and_pack(N, dense_on, wps, with_pack, dev):
    c = _partition_case(N, dense_on)
    new, pack = _partition_ref(c)
    sp, ns = c["sp"], c["n_splits"]
    max_splits = len(sp["feat"])
    assert ns < max_splits

    def run(dv):
        rn = _t(c["row_node"], dv)
        assert rn.data_ptr() % 16 == 0
        counts = _t(np.array([ns, 77, 77], np.int32), dv)
        pk = torch.full((N,), S32, dtype=torch.int32, device=dv) if with_pack else None
        native.lib().tree_partition_cols(
            rn, _t(c["default_child"], dv), *(_t(sp[k], dv) for k in ("feat", "dflt", "other", "bin", "lid")), counts,
            _t(c["colptr"], dv), _t(c["csc_row"], dv), _t(c["csc_bin"], dv), _t(c["node_dense"], dv),
            _t(c["dense"], dv), max_splits, wps, _t(c["pack_slot"], dv) if with_pack else None,
            _t(c["pack_dig"], dv) if with_pack else None, pk)
        out = dict(row_node=_np(rn))
        if with_pack:
            out["pack"] = _np(pk).view(np.uint32)
        return out

    def verify(o):
        _partition_verify(c, new, o)
        if with_pack:
            assert np.array_equal(o["pack"], pack), np.flatnonzero(o["pack"] != pack)[:8]
            if N == 4099:
                assert (pack & 0xFF == 0xFF).any() and (pack & 0xFF == 254).any()

    _check(dev, run, verify)


# ---------------------------------------------------------------------------- sibling subtraction
@functools.lru_cache(maxsize=None)
def _subtract_case(TB):
    rng = np.random.default_rng(TB)
    # |parent| <= 2^62 and |sibling| <= 2^61: the difference stays inside int64
    parent = rng.integers(-2 ** 62, 2 ** 62, (3, TB, 2), dtype=np.int64, endpoint=True)
    parent[0, 0], parent[1, -1] = (2 ** 62, -2 ** 62), (-2 ** 62, 2 ** 62)
    cur = rng.integers(-2 ** 61, 2 ** 61, (8, TB, 2), dtype=np.int64, endpoint=True)
    cur[1, 0], cur[3, -1] = (-2 ** 61, 2 ** 61), (2 ** 61, -2 ** 61)
    dst = np.array([0, 2, -1, 5], np.int32)    # rows 4, 6, 7 of cur: named by nothing
    par = np.array([0, 0, 2, 1], np.int32)     # two pairs share parent 0; the padded triple's
    sib = np.array([1, 3, 6, 3], np.int32)     # parent and sibling are in range but meaningless
    return parent, cur, dst, par, sib


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("TB", [1, 255, 256, 257, 1024 * 256 + 3])
def test_hist_subtract(TB, dev):
    parent, cur, dst, par, sib = _subtract_case(TB)
    want = cur.copy()
    for d, p, s in zip(dst, par, sib):
        if d >= 0:
            want[d] = parent[p] - cur[s]       # (exact: see the ranges above)
    assert want[0, 0].tolist() == [2 ** 62 + 2 ** 61, -2 ** 62 - 2 ** 61]

    def run(dv):
        cu = _t(cur, dv)
        native.lib().tree_hist_subtract(_t(parent, dv), cu, _t(dst, dv), _t(par, dv), _t(sib, dv), TB)
        return dict(cur=_np(cu))

    def verify(o):
        assert np.array_equal(o["cur"], want)
        for r in (1, 3, 4, 6, 7):              # siblings and unnamed rows keep their contents
            assert np.array_equal(o["cur"][r], cur[r])

    _check(dev, run, verify)


# --------------------------------------------------------------------------- best split per node
QNAN = 0x7FF8000000000000


def _best_scenarios(Fa, rng):
    """gain rows [Fa] that put the maximum, ties, NaN and infinities where the 1024-thread,
    4-features-per-thread search can go wrong"""
    base = lambda: -np.abs(rng.standard_normal(Fa)) - 1.0
    out = {}

    def put(name, pairs):
        g = base()
        for f, v in pairs:
            if not 0 <= f < Fa:
                return
        for f, v in pairs:
            g[f] = v
        out[name] = g

    put("maximum at the last feature", [(Fa - 1, 2.5)])
    put("tie (f, f + 1024)", [(5, 3.0), (5 + 1024, 3.0)])
    put("tie (f, f + 1)", [(Fa // 2, 3.0), (Fa // 2 + 1, 3.0)])
    put("tie (1023, 1024)", [(1023, 3.0), (1024, 3.0)])
    put("tie (Fa - 1, 0)", [(Fa - 1, 3.0), (0, 3.0)])
    put("tie of three", [(Fa - 1, 3.0), (Fa // 3, 3.0), (Fa // 3 + 2048, 3.0)])
    out["every gain -inf"] = np.full(Fa, -np.inf)
    put("NaN in the last feature", [(0, 7.0), (Fa - 1, np.nan)])
    put("+inf", [(Fa - 1, np.inf), (Fa // 2, 1e300)])
    put("+inf tie", [(Fa - 1, np.inf), (Fa // 2, np.inf)])
    g = np.full(Fa, -1.0)
    g[Fa - 1], g[Fa // 2] = 0.0, -0.0
    out["-0.0 before 0.0"] = g.copy()
    g[Fa - 1], g[Fa // 2] = -0.0, 0.0
    out["0.0 before -0.0"] = g
    out["plain"] = rng.standard_normal(Fa)
    return out


def _best_ref(gain, bins, left, f0):
    out = []
    for n, g in enumerate(gain):
        if np.isnan(g).any():
            bits, f = QNAN, 0
        else:
            f = int(np.flatnonzero(g == g.max())[0])           # value equality: the lowest feature
            bits = int(g[f:f + 1].view(np.uint64)[0])
        out.append([bits, f + f0, int(bins[n, f]), int(left[n, f, 0]), int(left[n, f, 1])])
    return np.array([[v - 2 ** 64 if v >= 2 ** 63 else v for v in row] for row in out], np.int64)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("Fa", [1, 63, 64, 1023, 1024, 1025, 4096, 4097])
def test_split_best(Fa, dev):
    rng = np.random.default_rng(Fa)
    sc = _best_scenarios(Fa, rng)
    names = list(sc)
    if Fa >= 4097:
        assert len(names) == 13                # every placement applies
    # single nodes, and groups of 5 nodes (a NaN or -inf node next to ordinary ones)
    groups = [[k] for k in names] + [[names[(i + j) % len(names)] for j in range(5)] for i in range(0, len(names), 3)]
    C = native.lib()
    f0 = 1000
    for grp in groups:
        gain = np.stack([sc[k] for k in grp])
        nodes = len(grp)
        bins = rng.integers(0, 255, (nodes, Fa)).astype(np.int32)
        left = rng.integers(-2 ** 62, 2 ** 62, (nodes, Fa, 2), dtype=np.int64)
        want = _best_ref(gain, bins, left, f0)
        for k, w in zip(grp, want):            # the reference itself on the spelled-out cases
            if k == "NaN in the last feature":
                assert w[0] == QNAN and w[1] == f0
            if k == "every gain -inf":
                assert w[1] == f0
            if k == "-0.0 before 0.0":
                assert w[0] == -2 ** 63 and w[1] == f0 + Fa // 2

        def run(dv):
            out = torch.full((nodes, 5), -99, dtype=torch.int64, device=dv)
            C.tree_split_best(_t(gain, dv), _t(bins, dv), _t(left, dv), f0, out)
            return dict(out=_np(out))

        def verify(o):
            assert np.array_equal(o["out"], want), (grp, o["out"].tolist(), want.tolist())

        _check(dev, run, verify)


# --------------------------------------------------------------------- gradient and leaf update
@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("N", [1, 257, 4099, 8192 * 256 + 3])
def test_leaf_update_is_one_fp64_add(N, dev):
    row_node, margin, value = (x[:N] if i < 2 else x for i, x in enumerate(_big_rows()))
    want = margin + value[row_node]

    def run(dv):
        m = _t(margin, dv)
        native.lib().tree_leaf_update(m, _t(row_node, dv), _t(value, dv))
        return dict(margin=_np(m))

    _check(dev, run, lambda o: np.testing.assert_array_equal(o["margin"].view(np.uint64), want.view(np.uint64)))


SPECIAL_MARGINS = [0.0, -0.0, 1e-300, -1e-300, 36.7, -36.7, 745.0, -745.0, 800.0, -800.0, 1e308, -1e308]


@functools.lru_cache(maxsize=None)
def _logistic_case(weighted):
    m1 = np.concatenate([SPECIAL_MARGINS, np.random.default_rng(4).standard_normal(4099) * 10])
    ws = [0.0, 0.5, 3.0] if weighted else [1.0]
    margin = np.tile(m1, 2 * len(ws))
    label = np.repeat([0.0, 1.0], len(m1) * len(ws)).astype(np.float32)
    weight = np.tile(np.repeat(ws, len(m1)), 2).astype(np.float32)
    L = np.longdouble
    with np.errstate(over="ignore", under="ignore"):
        p = 1 / (1 + np.exp(-margin.astype(L)))
    w = weight.astype(L)
    gs = (p - label.astype(L)) * w
    hs = np.maximum(p * (1 - p), L(1e-16)) * w
    return margin, label, weight, gs, hs


def _ulp32(x):
    """spacing of float32 at |x| (longdouble array): 2^(floor(log2 |x|) - 23), 2^-149 at the bottom"""
    _, e = np.frexp(np.abs(x))
    e = np.where(x == 0, -200, e - 1)
    return np.ldexp(np.longdouble(1.0), np.maximum(e, -126) - 23)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("weighted", [False, True])
def test_logistic_grad(weighted, dev):
    """|g - g*| <= half an fp32 ulp (the final rounding) + 8 * 2^-53 * |w| (exp, the divide and the
    subtract in fp64; the cancellation in p - y does not shrink that error). Derived, not measured."""
    margin, label, weight, gs, hs = _logistic_case(weighted)
    N = len(margin)
    g = torch.full((N,), 7.0, dtype=torch.float32, device=dev)
    h = torch.full((N,), 7.0, dtype=torch.float32, device=dev)
    native.lib().tree_logistic_grad(_t(margin, dev), _t(label, dev), _t(weight, dev) if weighted else None, g, h)
    g, h = _np(g), _np(h)
    slack = 8 * np.longdouble(2.0) ** -53 * np.abs(weight.astype(np.longdouble))
    for got, want, name in ((g, gs, "g"), (h, hs, "h")):
        err = np.abs(got.astype(np.longdouble) - want)
        bound = 0.5 * _ulp32(want) + slack
        worst = int(np.argmax(err - bound))
        print(f"{name}: worst err - bound = {float(err[worst] - bound[worst]):.3e} at margin {margin[worst]!r}")
        assert (err <= bound).all(), (name, margin[worst], float(got[worst]), float(want[worst]))
    w64, y64 = weight.astype(np.float64), label.astype(np.float64)
    for m, p in ((800.0, 1.0), (-800.0, 0.0)):             # exp underflows / overflows: p is exactly 1 / 0
        i = margin == m
        assert i.sum() == 2 * (3 if weighted else 1)
        assert np.array_equal(h[i], (np.float64(1e-16) * w64[i]).astype(np.float32))
        assert np.array_equal(g[i], ((p - y64[i]) * w64[i]).astype(np.float32))
