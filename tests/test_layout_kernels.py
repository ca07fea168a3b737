"""The layout build under every tree model, kernel by kernel against plain numpy: the feature-major
CSC of ``feature_order`` (``csc_row``, ``csc_cnt``, ``colptr``, ``df``, ``maxc``), ``clamp_u8``,
``copy_segments``, ``dense_scatter``, ``block_bounds``, ``pack_runs``, the count path of ``quantize``
and the device build of the histogram CSC and its work items (``csrc/sort_kernels.hip`` and the host
twins in ``csrc/sparse_cpu.cpp``). Everything is integer: every comparison is exact. The references
are written here and call none of the project's native code."""
import functools

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.models import quantize as qmod
from fraud_detection_spark_kafka_llm_amd.ops import native
from fraud_detection_spark_kafka_llm_amd.ops.sparse import FeatureOrder, IncrementalFeatureOrder, feature_order

GPU = pytest.param("cuda:0", marks=pytest.mark.gpu)
DEVS = ["cpu", GPU]
BLOCK_CAP = 16384 * 256            # entries one launch covers before the kernels loop (grid_for)

INT_POOL = np.array([0, 1, 2, 254, 255, 256, 1000, -3, 2 ** 31 - 1], dtype=np.int64)
FLOAT_POOL = np.array([0.0, 0.5, 1.0, 254.9, 255.0, 300.5, -1.0], dtype=np.float64)
OUTPUTS = (("csc_row", np.int32), ("csc_cnt", np.uint8), ("colptr", np.int64), ("df", np.int64), ("maxc", np.int32))


# ------------------------------------------------------------------------------ the reference
def _b(c):
    """b(c) = 0 if c <= 0 else 255 if c >= 255 else floor(c), on the count as it is stored."""
    c = np.asarray(c).astype(np.float64)
    return np.where(c <= 0, 0.0, np.where(c >= 255, 255.0, np.floor(np.minimum(c, 255.0)))).astype(np.uint8)


def _ref_order(indptr, idx, cnt, F):
    row = np.repeat(np.arange(indptr.size - 1, dtype=np.int32), np.diff(indptr))
    order = np.argsort(idx, kind="stable")
    b = _b(cnt)
    lens = np.bincount(idx, minlength=F)
    colptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cb = b[order]
    maxc = np.zeros(F, dtype=np.int32)
    full = lens > 0
    if full.any():          # (the empty columns left out, every start is the end of the column before)
        maxc[full] = np.maximum.reduceat(cb, colptr[:-1][full])
    df = np.bincount(idx[b > 0], minlength=F).astype(np.int64)
    return dict(csc_row=row[order], csc_cnt=cb, colptr=colptr, df=df, maxc=maxc)


def _check(fo, ref, what=""):
    for k, dt in OUTPUTS:
        got = getattr(fo, k).cpu().numpy()
        assert got.dtype == dt and got.shape == ref[k].shape and np.array_equal(got, ref[k]), f"{what} {k}"


def _order(dev, indptr, idx, cnt, F, **kw):
    return feature_order(torch.tensor(indptr).to(dev), torch.tensor(idx).to(dev), torch.tensor(cnt).to(dev), F, **kw)


def _counts(n, dtype, seed, every=False):
    """Counts drawn from the pool of the dtype; ``every``: each value of the pool must occur."""
    pool = (INT_POOL if np.dtype(dtype) == np.int32 else FLOAT_POOL).astype(dtype)
    c = pool[np.random.default_rng(seed).integers(0, pool.size, n)]
    assert not every or set(np.unique(c).tolist()) == set(pool.tolist())
    return c


# ------------------------------------------------------------------------------ feature_order
ROWS, FEATS = 1027, 700
ABSENT = (1, 349, 350, 351, FEATS - 2)


@functools.lru_cache(maxsize=None)
def _hand_pattern():
    """(indptr, idx): row lengths cycle through 0, 1, 63, 64, 65, 129, 300 (below, at and above one
    and two 64-lane passes), the first and the last row are empty, every other row stores feature 0
    (its key run spans many waves and several workgroups), rows of two or more entries store the last
    feature too; features 1, 349..351 and F - 2 are stored nowhere."""
    assert ROWS % 4 == 3
    rng = np.random.default_rng(33)
    lens = np.array([(0, 1, 63, 64, 65, 129, 300)[i % 7] for i in range(ROWS)])
    lens[-1] = 0
    mid = np.setdiff1d(np.arange(2, FEATS - 2), ABSENT)
    idx = []
    for n in lens:
        ends = [0][:n] + [FEATS - 1][:max(n - 1, 0)]
        idx.append(np.sort(np.concatenate([ends, rng.choice(mid, max(n - 2, 0), replace=False)])).astype(np.int32))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(idx)
    present = np.bincount(idx, minlength=FEATS) > 0
    assert lens[0] == 0 and lens[-1] == 0 and present[0] and present[-1] and not present[list(ABSENT)].any()
    assert np.bincount(idx, minlength=FEATS)[0] == int((lens > 0).sum()) > 3 * 256
    indptr.setflags(write=False)
    idx.setflags(write=False)
    return indptr, idx


@functools.lru_cache(maxsize=None)
def _hand_case(dtype, shift):
    """The hand-built CSR with counts of ``dtype``; ``shift``: the same matrix moved by +2 into
    F + 5 features (the first two and the last three features absent). With its reference."""
    indptr, idx = _hand_pattern()
    cnt = _counts(idx.size, dtype, 7, every=True)
    F = FEATS + 5 if shift else FEATS
    idx = (idx + 2).astype(np.int32) if shift else idx
    ref = _ref_order(indptr, idx, cnt, F)
    if shift:
        assert ref["colptr"][2] == 0 and ref["colptr"][-4] == idx.size
    assert 0 < ref["df"].sum() < idx.size and ref["maxc"].max() == 255
    return indptr, idx, cnt, F, ref


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("dtype", ["int32", "float32", "float64"])
def test_feature_order_hand_csr_equals_reference(dev, shift, dtype):
    indptr, idx, cnt, F, ref = _hand_case(dtype, shift)
    _check(_order(dev, indptr, idx, cnt, F), ref)


WAVE_LENS = (63, 1, 64, 65, 127, 129, 256, 257)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("at", ["first", "last"])
def test_feature_order_maximum_at_the_ends_of_runs_that_cross_waves(dev, at):
    """Column f holds rows 0 .. len_f - 1, so the key runs start and end below, at and above the
    64-entry waves of the segmented maximum; a column's maximum is stored once, at its first or at
    its last entry. The last stored column holds zero counts only."""
    lens = np.array(WAVE_LENS + (100,))
    F = lens.size + 1                                     # (and one absent feature behind them)
    n = int(lens.max()) + 1
    has = np.arange(n)[:, None] < lens[None, :]
    indptr = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64)
    row, idx = np.nonzero(has)
    top = 10 + 20 * np.arange(lens.size)                  # the unique maximum of column f
    cnt = np.random.default_rng(5).integers(0, 10, idx.size)      # every other count is smaller
    pos = np.zeros(lens.size, dtype=np.int64) if at == "first" else lens - 1
    here = row == pos[idx]
    cnt[here] = top[idx[here]]
    cnt[idx == lens.size - 1] = 0
    idx, cnt = idx.astype(np.int32), cnt.astype(np.int32)
    ref = _ref_order(indptr, idx, cnt, F)
    assert ref["maxc"].tolist() == top[:-1].tolist() + [0, 0] and ref["df"][-2] == 0
    assert np.diff(ref["colptr"]).tolist() == lens.tolist() + [0]
    for f in range(lens.size - 1):                        # the maximum occurs once, where it was put
        col = ref["csc_cnt"][ref["colptr"][f]:ref["colptr"][f + 1]]
        assert np.flatnonzero(col == top[f]).tolist() == [0 if at == "first" else lens[f] - 1]
    _check(_order(dev, indptr, idx, cnt, F), ref)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("F", [1, 2, 3, 64, 65])
def test_feature_order_small_feature_spaces(dev, F):
    """1, 1, 2, 6 and 7 key bits of the radix sort."""
    rng = np.random.default_rng(100 + F)
    has = rng.random((200, F)) < 0.4
    has[0] = has[-1] = False
    has[7] = True
    indptr = np.concatenate([[0], np.cumsum(has.sum(1))]).astype(np.int64)
    idx = np.nonzero(has)[1].astype(np.int32)
    cnt = _counts(idx.size, np.int32, F)
    _check(_order(dev, indptr, idx, cnt, F), _ref_order(indptr, idx, cnt, F))


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("dtype", ["int32", "float32", "float64"])
def test_feature_order_of_an_empty_csr(dev, dtype):
    F = 7
    indptr, idx, cnt = np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=dtype)
    fo = _order(dev, indptr, idx, cnt, F)
    ref = _ref_order(indptr, idx, cnt, F)
    assert not ref["colptr"].any() and not ref["df"].any() and not ref["maxc"].any()
    _check(fo, ref)


@pytest.mark.gpu
def test_gpu_feature_order_past_the_block_cap():
    """More entries than one launch of 16384 workgroups covers: unpack, colptr and the feature
    statistics take their grid-stride loops, with three key runs of over a million entries each."""
    nnz = BLOCK_CAP + 70
    F, feats = 700, np.array([3, 350, 699], dtype=np.int32)
    rows = (nnz // 12 + 2) * 7                            # rows r store the subset r % 7 + 1 of feats: 12 per 7
    has = (((np.arange(rows) % 7 + 1)[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)
    idx = np.broadcast_to(feats, (rows, 3))[has][:nnz].copy()
    indptr = np.minimum(np.concatenate([[0], np.cumsum(has.sum(1))]), nnz).astype(np.int64)
    assert idx.size == nnz == indptr[-1] and np.diff(indptr).max() == 3
    cnt = np.random.default_rng(1).integers(0, 3, nnz).astype(np.int32)
    cnt[0], cnt[-1] = 200, 255
    ref = _ref_order(indptr, idx, cnt, F)
    assert ref["df"].sum() > nnz // 2 and sorted(ref["maxc"][feats].tolist()) == [2, 200, 255]
    _check(_order("cuda:0", indptr, idx, cnt, F), ref)


def _same(a, b, what):
    for k, _ in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what} {k}"


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("dtype", ["int32", "float32"])
def test_row_blocked_order_equals_one_shot_with_zero_and_fractional_counts(dev, dtype):
    """``df`` counts the entries whose clamped count is positive on every path: stored zeros,
    negative counts and fractions below 1 leave it, however the rows are cut into blocks."""
    indptr, idx, cnt, F, ref = _hand_case(dtype, False)
    assert (ref["df"] < np.diff(ref["colptr"])).any()
    ip, ix, c = (torch.tensor(a).to(dev) for a in (indptr, idx, cnt))
    one = feature_order(ip, ix, c, F)
    _check(one, ref, "one-shot")
    for blk in (300, 7777, 50000):
        assert idx.size > blk
        got = feature_order(ip, ix, c, F, block_entries=blk)
        _same(got, one, f"block_entries={blk}")
        _check(got, ref, f"block_entries={blk}")


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("dtype", ["int32", "float32"])
def test_incremental_order_equals_one_shot_with_zero_and_fractional_counts(dev, dtype):
    """Uneven cuts, a single block (the shortcut of ``finish``) and blocks of one row."""
    indptr, idx, cnt, F, ref = _hand_case(dtype, False)
    ip, ix, c = (torch.tensor(a).to(dev) for a in (indptr, idx, cnt))
    one = feature_order(ip, ix, c, F)
    for cuts in ([0, ROWS], [0, 1, 300, 301, 900, ROWS], [0, 500, ROWS], [0, 2, 3, 1026, ROWS]):
        inc = IncrementalFeatureOrder(F, dev)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            e0, e1 = int(indptr[r0]), int(indptr[r1])
            inc.add(ip[r0:r1 + 1] - e0, ix[e0:e1], c[e0:e1], r0)
        got = inc.finish()
        _same(got, one, f"cuts={cuts}")
        _check(got, ref, f"cuts={cuts}")


# ------------------------------------------------------------------------------ clamp_u8
SENTINEL = 0xA5


def _clamp_case(dev, n, maxvs):
    src = (np.arange(n) % 256).astype(np.uint8)
    x = torch.from_numpy(src).to(dev)
    for maxv in maxvs:
        out = torch.full((n + 37,), SENTINEL, dtype=torch.uint8, device=dev)
        native.lib().clamp_u8(x, maxv, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], np.minimum(src, maxv)), (n, maxv)
        assert (got[n:] == SENTINEL).all(), (n, maxv)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 4101])
@pytest.mark.parametrize("maxv", [0, 1, 31, 254, 255])
def test_clamp_u8_equals_minimum_and_leaves_the_bytes_behind(dev, n, maxv):
    _clamp_case(dev, n, [maxv])


@pytest.mark.gpu
def test_gpu_clamp_u8_past_the_block_cap():
    """One 16-byte vector more than a launch of 16384 workgroups covers, and a 5-byte tail."""
    _clamp_case("cuda:0", BLOCK_CAP * 16 + 21, [0, 1, 31, 254, 255])


# ------------------------------------------------------------------------------ copy_segments
def _copy_case(dev, lens, src_start, dst_start, n_src, n_dst, add):
    """dst[dst_start[i] + k] = (src_row, uint8(src_key + add[i]))[src_start[i] + k], k < lens[i]; the
    rest of dst keeps its sentinels."""
    rng = np.random.default_rng(int(n_src))
    lens, src_start, dst_start = (np.asarray(a, dtype=np.int64) for a in (lens, src_start, dst_start))
    assert (src_start + lens <= n_src).all() and (dst_start + lens <= n_dst).all()
    src_row = rng.integers(-2 ** 31, 2 ** 31, n_src).astype(np.int32)
    src_key = (np.arange(n_src) * 7 % 256).astype(np.uint8)
    want_row, want_key = np.full(n_dst, -7, dtype=np.int32), np.full(n_dst, 0xEE, dtype=np.uint8)
    rep = np.repeat(np.arange(lens.size), lens)
    k = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    assert np.unique(dst_start[rep] + k).size == k.size               # the segments do not overlap in dst
    want_row[dst_start[rep] + k] = src_row[src_start[rep] + k]
    a = np.zeros(lens.size, dtype=np.int64) if add is None else np.asarray(add, dtype=np.int64)
    sums = src_key[src_start[rep] + k].astype(np.int64) + a[rep]
    want_key[dst_start[rep] + k] = (sums & 0xFF).astype(np.uint8)
    assert add is None or (sums > 255).any()
    assert (want_row == -7).sum() >= n_dst - k.size > 0
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    dst_row, dst_key = T(np.full(n_dst, -7, dtype=np.int32)), T(np.full(n_dst, 0xEE, dtype=np.uint8))
    native.lib().copy_segments(T(src_row), T(src_key), T(src_start), T(dst_start), T(lens), dst_row, dst_key,
                               None if add is None else T(np.asarray(add, dtype=np.uint8)))
    assert np.array_equal(dst_row.cpu().numpy(), want_row)
    assert np.array_equal(dst_key.cpu().numpy(), want_key)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("with_add", [False, True])
def test_copy_segments_lengths_around_the_workgroup_and_the_piece(dev, with_add):
    lens = np.array([257, 0, 8193, 1, 256, 8192, 255, 0])
    order = np.array([5, 2, 7, 0, 6, 1, 4, 3])                        # places in dst, with a gap before each
    dst_start = np.zeros(lens.size, dtype=np.int64)
    pos = 3
    for i in order:
        dst_start[i] = pos
        pos += lens[i] + 5
    src_order = np.array([3, 6, 0, 4, 1, 7, 2, 5])
    src_start = np.zeros(lens.size, dtype=np.int64)
    p = 11
    for i in src_order:
        src_start[i] = p
        p += lens[i] + 2
    _copy_case(dev, lens, src_start, dst_start, p + 9, pos + 4, [0, 9, 255, 200, 1, 128, 77, 3] if with_add else None)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("with_add", [False, True])
def test_copy_segments_more_segments_than_workgroups(dev, with_add):
    """65536 + 7 short segments: the device walks them in a grid-stride loop."""
    nseg = 65536 + 7
    lens = np.arange(nseg) * 7 % 4
    src_start = np.cumsum(lens) - lens
    back = lens[::-1]
    dst_start = (np.cumsum(back + 1) - back)[::-1].copy()             # reversed order, one free slot before each
    _copy_case(dev, lens, src_start, dst_start, int(lens.sum()) + 1, int(lens.sum()) + nseg + 1,
               np.arange(nseg) * 37 % 256 if with_add else None)


# ------------------------------------------------------------------------------ dense_scatter
BIG_SEG = 65536 + 300


def _scatter_case(dev, lens):
    lens = np.asarray(lens, dtype=np.int64)
    big = int(lens.max()) > 256
    n_rows = BIG_SEG + 4 if big else 300
    n_pad = (n_rows + 63) // 64 * 64
    assert n_pad % 64 == 0 and n_pad >= BIG_SEG * big and n_pad > n_rows
    rng = np.random.default_rng(int(lens.sum()) + lens.size)
    rows = [np.delete(np.arange(n_rows), [0, 77, 40000, n_rows - 1]) if n == BIG_SEG else
            np.sort(rng.choice(n_rows, int(n), replace=False)) for n in lens]
    # the segments lie in the CSC in another order than in the block, with other entries between them
    place = rng.permutation(lens.size)
    seg_src = np.zeros(lens.size, dtype=np.int64)
    pos = 5
    for i in place:
        seg_src[i] = pos
        pos += lens[i] + 3
    csc_row = rng.integers(0, n_rows, pos + 16).astype(np.int32)
    csc_bin = rng.integers(0, 64, pos + 16).astype(np.uint8)
    zero_bin = (200 + np.arange(lens.size)).astype(np.uint8)          # a distinct prefill per row of the block
    want = np.repeat(zero_bin[:, None], n_pad, axis=1)
    for i, r in enumerate(rows):
        csc_row[seg_src[i]:seg_src[i] + lens[i]] = r
        want[i, r] = csc_bin[seg_src[i]:seg_src[i] + lens[i]]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    dense = T(np.repeat(zero_bin[:, None], n_pad, axis=1))
    native.lib().dense_scatter(T(csc_row), T(csc_bin), T(seg_src), T(lens), dense, int(lens.max()))
    got = dense.cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[:, n_rows:] == zero_bin[:, None]).all()               # the pad columns


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("n", [0, 1, 256, BIG_SEG])
def test_dense_scatter_of_one_segment(dev, n):
    _scatter_case(dev, [n])


@pytest.mark.parametrize("dev", DEVS)
def test_dense_scatter_of_five_segments(dev):
    _scatter_case(dev, [256, 0, BIG_SEG, 1, 256])


# ------------------------------------------------------------------------------ block_bounds
@functools.lru_cache(maxsize=None)
def _bounds_columns():
    """150 columns of sorted rows over 400 rows: an empty one, one inside a single block of 50,
    one with rows at the multiples of 50 and one below them, a full one, random ones."""
    rng = np.random.default_rng(12)
    n_rows, ncol = 400, 150
    cols = [np.zeros(0, dtype=np.int64), np.arange(51, 61), np.sort(np.concatenate([np.arange(0, 400, 50),
                                                                                 np.arange(49, 400, 50)])),
            np.arange(n_rows)]
    for f in range(4, ncol):
        cols.append(np.flatnonzero(rng.random(n_rows) < rng.choice([0.0, 0.01, 0.2, 0.9])))
    colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    subset = np.concatenate([[3, 0, 2, 1], 4 + rng.permutation(ncol - 4)[:127]]).astype(np.int32)
    subset = subset[rng.permutation(subset.size)]
    assert np.unique(subset).size == subset.size == 131 and (np.diff(subset) < 0).any()
    return n_rows, cols, colptr, np.concatenate(cols).astype(np.int32), subset


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("nblk,row_block", [(1, 400), (1, 50), (3, 50), (3, 134), (8, 50), (8, 60)])
def test_block_bounds_equal_searchsorted(dev, nblk, row_block):
    n_rows, cols, colptr, csc_row, subset = _bounds_columns()
    total = subset.size * (nblk + 1)
    assert total > 256 and total % 256 != 0        # (3 x 134 and 8 x 60 rows reach past the 400 rows)
    want = np.stack([colptr[c] + np.searchsorted(cols[c], np.arange(nblk + 1) * row_block, "left") for c in subset])
    bounds = torch.full((subset.size, nblk + 1), -1, dtype=torch.int64, device=dev)
    T = lambda x: torch.tensor(x).to(dev)   # noqa: E731
    native.lib().block_bounds(T(csc_row), T(colptr), T(subset), nblk, row_block, bounds)
    assert np.array_equal(bounds.cpu().numpy(), want)


# ------------------------------------------------------------------------------ pack_runs (host)
def _ref_pack_runs(packable, stride, ncol, pack_keys, max_entries):
    """Greedy runs of consecutive packable features: a run takes the next feature while its keys
    (features x the run's largest stride) stay <= pack_keys and its entries <= max_entries; a
    feature that fits no run alone is skipped. Rows (first, end, log2 of the stride)."""
    out, i = [], 0
    while i < len(packable):
        j, st, ent = i, 0, 0
        while j < len(packable) and packable[j]:
            s2 = max(st, int(stride[j]))
            if (j - i + 1) * s2 > pack_keys or ent + int(ncol[j]) > max_entries:
                break
            st, ent, j = s2, ent + int(ncol[j]), j + 1
        if j == i:
            i += 1
            continue
        out.append((i, j, (st - 1).bit_length()))
        i = j
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def _pack_runs(packable, stride, ncol, pack_keys, max_entries):
    return native.lib().pack_runs(torch.tensor(packable, dtype=torch.uint8), torch.tensor(stride, dtype=torch.int64),
                                  torch.tensor(ncol, dtype=torch.int64), pack_keys, max_entries).numpy()


def test_pack_runs_equal_the_greedy_loop():
    #            lone over keys | lone over entries | stride grows in the run | blocked | 9 x stride 2 | entries
    packable = [1,                1,                  1, 1, 1, 1, 1,            0,        1, 1, 1, 1, 1, 1, 1, 1, 1,
                0, 0, 1, 1, 1, 1]
    stride = [32,                 2,                  2, 2, 4, 2, 8,            2,        2, 2, 2, 2, 2, 2, 2, 2, 2,
              2, 2, 4, 4, 4, 4]
    ncol = [1,                    101,                1, 1, 1, 1, 1,            1,        1, 1, 1, 1, 1, 1, 1, 1, 1,
            1, 1, 40, 40, 40, 5]
    got = _pack_runs(packable, stride, ncol, 16, 100)
    want = np.array([[2, 6, 2],        # 4 features at stride 4 = 16 keys; the fifth would raise the stride to 8
                     [6, 7, 3],
                     [8, 16, 1],       # 8 x 2 keys: the limit on keys
                     [16, 17, 1],
                     [19, 21, 2],      # 40 + 40 entries: the third would pass 100
                     [21, 23, 2]])
    assert np.array_equal(_ref_pack_runs(packable, stride, ncol, 16, 100), want)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert _pack_runs([], [], [], 16, 100).shape == (0, 3)
    rng = np.random.default_rng(8)
    for _ in range(50):
        n = int(rng.integers(1, 80))
        p, s, c = rng.random(n) < 0.8, 2 ** rng.integers(1, 6, n), rng.integers(0, 60, n)
        keys, ents = int(rng.choice([4, 16, 64])), int(rng.choice([50, 100, 1000]))
        assert np.array_equal(_pack_runs(p.tolist(), s.tolist(), c.tolist(), keys, ents),
                              _ref_pack_runs(p, s, c, keys, ents))


# ------------------------------------------------------------------------------ quantize, count path
def _csr_of(dense):
    row, idx = np.nonzero(dense)
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(1))]).astype(np.int64)
    return indptr, idx.astype(np.int32), dense[row, idx]


@functools.lru_cache(maxsize=None)
def _count_matrix():
    """257 x 24 integer counts up to 300: column 0 in every row, columns 5 and 23 empty, column 9
    with counts of 1 only."""
    rng = np.random.default_rng(3)
    n, F = 257, 24
    dense = (rng.random((n, F)) < np.linspace(0.02, 0.7, F)) * rng.integers(1, 301, (n, F))
    dense[:, 0] = rng.integers(1, 301, n)
    dense[:, [5, 23]] = 0
    dense[:, 9] = rng.random(n) < 0.3
    assert dense.max() == 300
    dense.setflags(write=False)
    return dense


def _tail(view):
    """The CSC_PAD entries behind ``view``, read through the view's own storage."""
    n = int(view.numel())
    return view.as_strided((n + qmod.CSC_PAD,), (1,))[n:].cpu().numpy()


def _check_count_quantized(Q, dense, scale, max_bins):
    active = np.flatnonzero((dense.max(0) > 0) & (scale > 0))
    top = max_bins - 1
    assert np.array_equal(Q.fid_orig.cpu().numpy(), active) and Q.n_rows == dense.shape[0]
    nb = np.minimum(dense[:, active].max(0), top) + 1
    assert np.array_equal(Q.nbins.cpu().numpy(), nb.astype(np.int32))
    colptr = np.concatenate([[0], np.cumsum((dense[:, active] > 0).sum(0))])
    assert np.array_equal(Q.colptr.cpu().numpy(), colptr)
    rows, bins = Q.csc_row.cpu().numpy(), Q.csc_bin.cpu().numpy()
    assert rows.size == bins.size == colptr[-1]
    for j, f in enumerate(active):
        r = rows[colptr[j]:colptr[j + 1]]
        assert np.array_equal(r, np.flatnonzero(dense[:, f]))                      # ascending, every stored row
        assert np.array_equal(bins[colptr[j]:colptr[j + 1]], np.minimum(dense[r, f], top).astype(np.uint8))
    want_thr = np.concatenate([(np.arange(b, dtype=np.float64) + 0.5) * scale[f] for f, b in zip(active, nb)])
    assert np.array_equal(Q.thresholds, want_thr)
    assert np.array_equal(Q.boff.cpu().numpy(), np.concatenate([[0], np.cumsum(nb)]))
    assert (_tail(Q.csc_bin) == 0xFF).all()


def _count_column(dev, scale, fo=None):
    dense = _count_matrix()
    indptr, idx, cnt = _csr_of(dense)
    T = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
    return VectorColumn.tfidf(dense.shape[1], T(indptr), T(idx), T(cnt.astype(np.int32)), T(scale), fo)


@pytest.mark.parametrize("dev", DEVS)
@pytest.mark.parametrize("max_bins", [2, 4, 256])
@pytest.mark.parametrize("zero_scales", [False, True])
def test_count_path_quantize_equals_a_dense_model(dev, max_bins, zero_scales):
    """``zero_scales``: features 0 (in every row), 7 and 8 have scale 0; their entries leave the CSC."""
    dense = _count_matrix()
    scale = np.random.default_rng(4).uniform(0.5, 2.0, dense.shape[1])
    if zero_scales:
        scale[[0, 7, 8]] = 0.0
    vc = _count_column(dev, scale)
    Q = qmod.quantize(vc, max_bins=max_bins, counts=vc.tf_counts, scale=vc.tf_scale)
    assert Q.device.type == torch.device(dev).type
    _check_count_quantized(Q, dense, scale, max_bins)


@pytest.mark.parametrize("dev", DEVS)
def test_count_path_quantize_drops_inactive_entries_by_segment_copy(dev, monkeypatch):
    """With an order that cannot be compacted in place (``drop_features`` switched off here), the
    entries of the scale-0 features leave through ``clamp_u8`` into a full buffer and one
    ``copy_segments`` of the active columns: the same CSC, and the pad behind it is still 0xFF."""
    monkeypatch.setattr(FeatureOrder, "drop_features", lambda self, drop: None)
    dense = _count_matrix()
    scale = np.random.default_rng(4).uniform(0.5, 2.0, dense.shape[1])
    scale[[0, 7, 8]] = 0.0
    vc = _count_column(dev, scale)
    Q = qmod.quantize(vc, max_bins=4, counts=vc.tf_counts, scale=vc.tf_scale)
    assert int(Q.colptr[-1]) < int((dense > 0).sum())
    _check_count_quantized(Q, dense, scale, 4)
    assert not _tail(Q.csc_row).any()


@pytest.mark.parametrize("dev", DEVS)
def test_count_path_quantize_with_a_misaligned_shared_order(dev):
    """A column whose shared feature order keeps ``csc_cnt`` as a view at byte offset 3 of a larger
    buffer (the device clamp realigns it) quantizes like the column alone."""
    dense = _count_matrix()
    scale = np.random.default_rng(4).uniform(0.5, 2.0, dense.shape[1])
    plain = _count_column(dev, scale)
    fo = feature_order(plain.indptr, plain.indices, plain.tf_counts, plain.size)
    n = int(fo.csc_cnt.numel())
    buf = torch.full((n + 3 + qmod.CSC_PAD,), 0x5A, dtype=torch.uint8, device=dev)
    buf[3:3 + n] = fo.csc_cnt
    cnt_view = buf[3:3 + n]
    assert cnt_view.data_ptr() % 16 == 3
    vc = _count_column(dev, scale, FeatureOrder(fo.csc_row, cnt_view, fo.colptr, fo.df, fo.maxc))
    Q = qmod.quantize(vc, max_bins=4, counts=vc.tf_counts, scale=vc.tf_scale)
    _check_count_quantized(Q, dense, scale, 4)
    R = qmod.quantize(plain, max_bins=4, counts=plain.tf_counts, scale=plain.tf_scale)
    for k in ("fid_orig", "nbins", "zbin", "boff", "colptr", "csc_row", "csc_bin"):
        assert torch.equal(getattr(Q, k), getattr(R, k)), k
    assert np.array_equal(Q.thresholds, R.thresholds)
    assert np.array_equal(buf.cpu().numpy()[:3], [0x5A] * 3) and (buf[3 + n:] == 0x5A).all()   # the buffer is only read


# ------------------------------------------------------------------------------ histogram CSC and items
@pytest.mark.gpu
@pytest.mark.parametrize("light", [0, 60])
@pytest.mark.parametrize("hot_density", [0.0, 0.3])
def test_gpu_histogram_csc_items_and_dense_block_equal_host(monkeypatch, light, hot_density):
    """``_build_items`` and ``_build_dense`` on the device against the host, with the copy split
    into 64-entry pieces (so the per-piece key bases are used)."""
    monkeypatch.setattr(qmod, "COPY_PIECE", 64)
    monkeypatch.setattr(qmod, "LIGHT_ENTRIES", light)
    rng = np.random.default_rng(2)
    n, F = 5000, 40
    dense = (rng.random((n, F)) < np.linspace(0.002, 0.6, F)) * rng.integers(1, 5, (n, F))
    indptr, idx, cnt = _csr_of(dense)
    Q = {}
    for dev in ("cpu", "cuda:0"):
        vc = VectorColumn(F, torch.from_numpy(indptr).to(dev), torch.from_numpy(idx).to(dev),
                          torch.from_numpy(cnt.astype(np.float64)).to(dev))
        Q[dev] = qmod.quantize(vc, max_bins=8, chunk=100, super_rows=700, hot_density=hot_density)
    h, d = Q["cpu"], Q["cuda:0"]
    assert d.h_row.is_cuda and h.n_super == d.n_super == 8
    assert h.kbase_host.any() and int(np.diff(h.colptr.numpy()).max()) > 8 * 64      # key bases, split segments
    for k in ("h_row", "h_key", "kbase", "colptr", "csc_row", "csc_bin"):
        assert torch.equal(getattr(h, k), getattr(d, k).cpu()), k
    assert (_tail(d.h_key) == 0xFF).all() and (_tail(h.h_key) == 0xFF).all()
    assert (h.dense is None) == (d.dense is None) == (hot_density == 0.0)
    if h.dense is not None:
        assert np.array_equal(h.hot, d.hot) and torch.equal(h.dense, d.dense.cpu())
    for name in ("groups", "hot_groups"):
        gh, gd = getattr(h, name), getattr(d, name)
        assert len(gh) == len(gd) and (name != "groups" or len(gh) > 0)
        for a, b in zip(gh, gd):
            assert a.bt == b.bt
            for k in ("item_start", "item_end", "item_f0", "item_meta", "item_blk"):
                assert torch.equal(getattr(a, k), getattr(b, k).cpu()), (name, a.bt, k)
    assert (len(h.hot_groups) > 0) == (hot_density > 0)
