"""Device paths vs their host twins: CSR scoring, SpMV / SpMV^T (LR training), docFreq, L-BFGS LR,
the reference training flow on the GPU, and GBDT checkpoint / fault / resume on the GPU. The sparse
kernels (one wave per row, 64-lane stride, 4 rows per block) also against numpy truths on a CSR
built by hand: empty rows, rows longer than a wave, a row count that is no multiple of 4."""
import functools

import numpy as np
import pytest
import torch

from fraud_detection_spark_kafka_llm_amd.ml.linalg import VectorColumn
from fraud_detection_spark_kafka_llm_amd.ml.tree_model import ensemble_arrays
from fraud_detection_spark_kafka_llm_amd.ops import sparse as S
from fraud_detection_spark_kafka_llm_amd.ops.text import LinearScorer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _csr(n=3000, F=500, density=0.04, seed=0):
    rng = np.random.default_rng(seed)
    dense = (rng.random((n, F)) < density) * rng.integers(1, 7, (n, F)).astype(np.float64)
    y = ((dense[:, 3] > 0) | (dense[:, 7] > 2)).astype(np.float64)
    return VectorColumn(F, dense=torch.from_numpy(dense)), y


def test_score_csr_lr_and_trees_bitwise():
    from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt

    vc, y = _csr()
    lr = LinearScorer(np.random.default_rng(1).standard_normal(vc.size), 0.3)
    assert torch.equal(S.score_csr(vc, lr), S.score_csr(vc.to(DEV), lr).cpu())
    res = fit_gbdt(vc, torch.from_numpy(y.astype(np.float32)), GBDTParams(n_estimators=8, max_depth=4), device="cpu")
    arr = ensemble_arrays(res.trees, "value", cmp_less=True)
    assert torch.equal(S.score_csr(vc, arr), S.score_csr(vc.to(DEV), arr).cpu())


def test_spmv_spmv_t_and_doc_freq():
    vc, _ = _csr(seed=3)
    ip, ix, v = vc.csr()
    x = torch.randn(vc.size, dtype=torch.float64)
    r = torch.randn(len(vc), dtype=torch.float64)
    d = [t.to(DEV) for t in (ip, ix, v)]
    torch.testing.assert_close(S.spmv(*d, x.to(DEV)).cpu(), S.spmv(ip, ix, v, x), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(S.spmv_t(*d, r.to(DEV), vc.size).cpu(), S.spmv_t(ip, ix, v, r, vc.size),
                               rtol=1e-12, atol=1e-12)
    assert torch.equal(S.doc_freq(d[1], d[2], vc.size).cpu(), S.doc_freq(ix, v, vc.size))


ROWS, FEATS = 1027, 700                       # 1027 % 4 == 3: the last block has one idle wave


@functools.lru_cache(maxsize=None)
def _hand_csr():
    """(indptr, idx, integer values, dense fp64 matrix). Row lengths cycle through 0, 1, 63, 64,
    65, 129, 300 (below, at and above one and two 64-lane passes), the first and the last row are
    empty, every other row stores feature 0, rows of two or more entries store the last feature
    too, and feature 350 is stored nowhere."""
    rng = np.random.default_rng(21)
    lens = np.array([(0, 1, 63, 64, 65, 129, 300)[i % 7] for i in range(ROWS)])
    lens[-1] = 0
    mid = np.delete(np.arange(1, FEATS - 1), 349)
    idx, val = [], []
    for n in lens:
        cols = [0][:n] + [FEATS - 1][:max(n - 1, 0)]
        cols = np.sort(np.concatenate([cols, rng.choice(mid, max(n - 2, 0), replace=False)])).astype(np.int32)
        idx.append(cols)
        val.append(rng.integers(1, 7, n).astype(np.float64))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx, val = np.concatenate(idx), np.concatenate(val)
    dense = np.zeros((ROWS, FEATS))
    dense[np.repeat(np.arange(ROWS), lens), idx] = val
    assert (dense[lens > 0, 0] > 0).all() and not dense[:, 350].any() and not dense[0].any() and not dense[-1].any()
    return indptr, idx, val, dense


def _hand_vc(dtype, dev):
    indptr, idx, val, _ = _hand_csr()
    return VectorColumn(FEATS, torch.from_numpy(indptr).to(dev), torch.from_numpy(idx).to(dev),
                        torch.from_numpy(val.astype(dtype)).to(dev))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spmv_spmv_t_and_lr_score_equal_dense_matmul(dtype):
    """Integer values, weights with at most 10 fractional bits and integer residuals: every partial
    sum is exact in fp64, so any summation order (lane strides, butterflies, fp64 atomics) gives
    the dense matmul's numbers exactly."""
    dense = _hand_csr()[3]
    rng = np.random.default_rng(22)
    x = rng.integers(-2048, 2049, FEATS) / 1024.0
    r = rng.integers(-3, 4, ROWS).astype(np.float64)
    assert (r == 0).sum() > 50 and (r[dense[:, 0] > 0] != 0).sum() > 500      # (column 0: maximum contention)
    vc = _hand_vc(dtype, DEV)
    ip, ix, v = vc.csr()
    assert v.dtype == torch.from_numpy(np.zeros(1, dtype)).dtype
    y = S.spmv(ip, ix, v, torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.array_equal(y, dense @ x)
    g = S.spmv_t(ip, ix, v, torch.from_numpy(r).to(DEV), FEATS).cpu().numpy()
    assert np.array_equal(g, dense.T @ r)
    lr = LinearScorer(x, 0.375)
    got = S.score_csr(vc, lr)
    assert np.array_equal(got.cpu().numpy()[:, 0], dense @ x + 0.375)
    assert torch.equal(got.cpu(), S.score_csr(_hand_vc(dtype, "cpu"), lr))


@functools.lru_cache(maxsize=None)
def _hand_trees():
    """(70 boosted trees + one tree written by hand, 3 forest trees), grown on the host. The
    boosted leaves are rounded to 10 fractional bits (their sums are then exact in any order) and
    every other tree's thresholds are rounded up to integers, so values equal to a threshold exist
    and the two comparison rules differ."""
    from fraud_detection_spark_kafka_llm_amd.ml.tree_model import Tree
    from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
    from fraud_detection_spark_kafka_llm_amd.models.tree import fit_forest

    dense = _hand_csr()[3]
    y = ((dense[:, 0] >= 3) ^ (dense[:, FEATS - 1] >= 4) ^ (dense[:, 5] > 0)).astype(np.float32)
    vc = _hand_vc(np.float64, "cpu")
    boosted = fit_gbdt(vc, torch.from_numpy(y), GBDTParams(n_estimators=70, max_depth=3), device="cpu").trees
    assert len(boosted) == 70
    for i, t in enumerate(boosted):
        t.stats = np.round(t.stats * 1024.0) / 1024.0
        if i % 2:
            t.threshold = np.ceil(t.threshold)
    # root on the first stored index, then the last stored index and a feature no row stores
    z = np.zeros(7)
    hand = Tree(np.array([0, FEATS - 1, 350, -1, -1, -1, -1], np.int32), np.array([3.0, 2.0, 0.0, 0, 0, 0, 0]),
                np.array([1, 3, 5, -1, -1, -1, -1], np.int32), np.array([2, 4, 6, -1, -1, -1, -1], np.int32),
                np.array([0, 0, 0, 0.5, -0.25, 2.0, -4.0]).reshape(7, 1), z, z - 1, z.astype(np.int64), z, 0)
    forest = fit_forest(vc, torch.from_numpy(y), num_trees=3, max_depth=4, bootstrap=True, feature_subset="sqrt",
                        seed=5, device="cpu").trees
    assert len(forest) >= 3 and forest[0].stats.shape[1] == 2
    return boosted + [hand], forest


def _walk_scores(trees, payload, cmp_less):
    """[ROWS, K]: per row, the sum over the trees of the leaf reached by the Python tree walk"""
    indptr, idx, val, _ = _hand_csr()
    arr = ensemble_arrays(trees, payload)                   # (the leaf payloads only; the walk is Tree.leaf_of)
    leaf = arr.leaf.reshape(-1, arr.K)
    off = np.concatenate([[0], np.cumsum([t.num_nodes for t in trees])])
    out = np.zeros((ROWS, arr.K))
    for r in range(ROWS):
        x = dict(zip(idx[indptr[r]:indptr[r + 1]].tolist(), val[indptr[r]:indptr[r + 1]].tolist()))
        for k, t in enumerate(trees):
            out[r] += leaf[off[k] + t.leaf_of(x, cmp_less)]
    return out


@pytest.mark.parametrize("cmp_less", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score_csr_trees_equal_python_walk(dtype, cmp_less):
    boosted, forest = _hand_trees()
    vc, host = _hand_vc(dtype, DEV), _hand_vc(dtype, "cpu")
    arr = ensemble_arrays(boosted, "value", cmp_less=cmp_less)          # 71 trees: more than one per lane
    assert arr.num_trees == 71 and {0, 350, FEATS - 1} <= set(arr.feat.tolist())
    got = S.score_csr(vc, arr).cpu()
    want = _walk_scores(tuple(boosted), "value", cmp_less)
    assert np.array_equal(got.numpy(), want)                            # dyadic leaves: exact
    assert torch.equal(got, S.score_csr(host, arr))
    if cmp_less:
        assert not np.array_equal(want, _walk_scores(tuple(boosted), "value", False))
    arr2 = ensemble_arrays(forest, "normalized", cmp_less=cmp_less)
    assert arr2.K == 2
    got2 = S.score_csr(vc, arr2).cpu()
    np.testing.assert_allclose(got2.numpy(), _walk_scores(tuple(forest), "normalized", cmp_less), rtol=1e-13, atol=0)
    assert torch.equal(got2, S.score_csr(host, arr2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_doc_freq_stored_zeros_negatives_and_block_cap(dtype):
    idx = np.array([3, 3, 0, 699, 3, 0, 5, 699, 5, 3], np.int32)
    val = np.array([1, 0, -2, 0, -0.0, 4, 0, -1, 0.5, 7], dtype)        # zeros are stored but not counted
    want = np.bincount(idx[val != 0], minlength=FEATS)
    assert want[[0, 3, 5, 699]].tolist() == [2, 2, 1, 1]
    got = S.doc_freq(torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV), FEATS)
    assert np.array_equal(got.cpu().numpy(), want)
    nnz = 8192 * 256 + 5                                                # past the 8192-block cap: the strided pass
    rng = np.random.default_rng(23)
    idx = np.array([3, 350, 699], np.int32)[rng.integers(0, 3, nnz)]
    val = rng.integers(-1, 2, nnz).astype(dtype)
    val[-5:] = 1
    want = np.bincount(idx[val != 0], minlength=FEATS)
    got = S.doc_freq(torch.from_numpy(idx).to(DEV), torch.from_numpy(val).to(DEV), FEATS)
    assert np.array_equal(got.cpu().numpy(), want) and want.sum() > nnz // 2


def test_logistic_regression_gpu_matches_host():
    from fraud_detection_spark_kafka_llm_amd.models.lr import train_logistic_regression

    vc, y = _csr(seed=4)
    a = train_logistic_regression(vc, y, max_iter=60, reg_param=0.01, device="cpu")
    b = train_logistic_regression(vc, y, max_iter=60, reg_param=0.01, device=DEV)
    np.testing.assert_allclose(np.asarray(b[0]), np.asarray(a[0]), rtol=1e-6, atol=1e-8)
    assert b[1] == pytest.approx(a[1], rel=1e-6, abs=1e-8)


def test_reference_training_flow_on_gpu(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd import train

    monkeypatch.setenv("FDX_DEVICE", DEV)
    res = train.main(["--data", "", "--synthetic", "1600", "--no-plots", "--out-dir", str(tmp_path)])
    for model in ("DecisionTree", "RandomForest", "XGBoost"):
        assert res[model]["Test"]["Accuracy"] > 0.95, (model, res[model])
    assert (tmp_path / "fraud_detection_model" / "metadata" / "part-00000").exists()


def test_gbdt_fault_and_resume_on_gpu(tmp_path, monkeypatch):
    from fraud_detection_spark_kafka_llm_amd.models.gbdt import GBDTParams, fit_gbdt
    from fraud_detection_spark_kafka_llm_amd.parallel.checkpoint import InjectedFault

    vc, y = _csr(seed=5)
    yt = torch.from_numpy(y.astype(np.float32))
    p = GBDTParams(n_estimators=9, max_depth=4)
    ref = fit_gbdt(vc, yt, p, device=DEV)
    ck = str(tmp_path / "ck")
    monkeypatch.setenv("FDX_FAULT", "tree:5")
    with pytest.raises(InjectedFault):
        fit_gbdt(vc, yt, p, device=DEV, checkpoint_dir=ck, checkpoint_every=3)
    monkeypatch.delenv("FDX_FAULT")
    res = fit_gbdt(vc, yt, p, device=DEV, checkpoint_dir=ck, checkpoint_every=3, resume=True)
    assert len(res.trees) == 9
    for a, b in zip(res.trees, ref.trees):
        np.testing.assert_array_equal(a.feature, b.feature)
        np.testing.assert_allclose(a.stats, b.stats, rtol=1e-12, atol=1e-15)
