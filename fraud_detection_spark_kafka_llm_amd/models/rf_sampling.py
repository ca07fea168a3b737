"""Random-forest per-node feature subsampling (X-10, K-14).

Spark samples exactly ``numFeaturesPerNode`` of the ``numFeatures`` feature indices without
replacement per node (``featureSubsetStrategy="auto"`` = ceil(sqrt(F)) for a forest;
/root/reference/fraud_detection_spark.py:67-74). Here every (tree, node, feature index) has a
counter-based priority (``feature_priority`` in csrc/tree.h, uniform in [0, 1)), and a node samples
the k features with the smallest priorities: exactly k, without replacement, no state, identical
on every rank and on host/device. ``node_thresholds`` finds each node's k-th smallest priority over
all F indices (the split kernel keeps a feature iff its priority <= the threshold);
``level_feature_mask`` is the union over the level's nodes, so histograms are only built for
features some node can actually split on.
"""
from __future__ import annotations

import math

import torch

_M = (1 << 64) - 1


def _u64(x: int) -> int:
    x &= _M
    return x - (1 << 64) if x >= (1 << 63) else x


_C1 = _u64(0x9E3779B97F4A7C15)
_C2 = _u64(0xBF58476D1CE4E5B9)
_C3 = _u64(0x94D049BB133111EB)


def _srl(x: torch.Tensor, s: int) -> torch.Tensor:
    return (x >> s) & ((1 << (64 - s)) - 1)


def mix64(x: torch.Tensor) -> torch.Tensor:
    x = x + _C1
    x = (x ^ _srl(x, 30)) * _C2
    x = (x ^ _srl(x, 27)) * _C3
    return x ^ _srl(x, 31)


def hash_uniform(a, b, c: torch.Tensor) -> torch.Tensor:
    """Vectorised twin of ``fdx::hash_uniform(a, b, c)`` (a, b scalars or tensors)."""
    x = mix64(torch.as_tensor(a, dtype=torch.int64, device=c.device) ^
              mix64(torch.as_tensor(b, dtype=torch.int64, device=c.device) ^ mix64(c)))
    return _srl(x, 11).to(torch.float64) * (1.0 / 9007199254740992.0)


def features_per_node(strategy: str, num_features: int) -> int:
    s = str(strategy).lower()
    if s in ("auto", "sqrt"):
        return int(math.ceil(math.sqrt(num_features)))
    if s == "all":
        return num_features
    if s == "onethird":
        return int(math.ceil(num_features / 3.0))
    if s == "log2":
        return max(1, int(math.ceil(math.log2(num_features))))
    v = float(s)
    return int(math.ceil(v * num_features)) if v <= 1.0 else min(num_features, int(v))


def _priorities(seed: int, tree_index: int, node: int, fid: torch.Tensor) -> torch.Tensor:
    a = _u64(int(seed) ^ 0x5BD1E995)
    b = _u64(((int(tree_index) & 0xFFFFFFFF) << 32) | (int(node) & 0xFFFFFFFF))
    return hash_uniform(a, b, fid)


def node_thresholds(num_features: int, seed: int, tree_index: int, nodes: list, k: int, dev) -> torch.Tensor:
    """[len(nodes)] float64: the k-th smallest priority of each node over feature indices 0..F-1
    (1.0 when k >= F: every feature)."""
    out = torch.ones(len(nodes), dtype=torch.float64, device=dev)
    if k >= num_features:
        return out
    fid = torch.arange(num_features, dtype=torch.int64, device=dev)
    for i, n in enumerate(nodes):
        out[i] = torch.kthvalue(_priorities(seed, tree_index, n, fid), k).values
    return out


def level_feature_mask(Q, seed: int, tree_index: int, nodes: list, thr: torch.Tensor) -> torch.Tensor:
    """[Fa] bool: active features sampled by at least one of ``nodes``."""
    fid = Q.fid_orig
    mask = torch.zeros(fid.numel(), dtype=torch.bool, device=fid.device)
    for i, n in enumerate(nodes):
        mask |= _priorities(seed, tree_index, n, fid) <= thr[i]
    return mask


def row_keep_mask(seed: int, round_index: int, row0: int, n: int, subsample: float, dev="cpu") -> torch.Tensor:
    """[n] bool: the rows a GBDT round keeps under row subsampling -- global row ``row0 + r`` is kept
    iff ``hash_uniform(seed, round, row0 + r) < subsample`` (``row_stats`` in csrc/tree.h; every row
    when ``subsample`` is 1). Stateless: the same on host and device, on every rank and at every
    world size."""
    if subsample >= 1.0:
        return torch.ones(n, dtype=torch.bool, device=dev)
    rows = torch.arange(int(row0), int(row0) + n, dtype=torch.int64, device=dev)
    return hash_uniform(_u64(int(seed)), _u64(int(round_index) & 0xFFFFFFFFFFFFFFFF), rows) < float(subsample)


# ---------------------------------------------------------------------------- GBDT column sampling
COL_TREE_KEY = 0xFFFFFFFF          # pseudo-node of the tree stage
COL_LEVEL_KEY = 0xFFFFFFFE         # ... of level 0's stage; level d uses COL_LEVEL_KEY - d


def column_counts(num_features: int, colsample_bytree: float, colsample_bylevel: float,
                  colsample_bynode: float) -> tuple:
    """(k_tree, k_level, k_node): features each nested stage keeps, ``max(1, int(fraction * n))`` of
    the n features the stage before it keeps (xgboost's column sampler); 0 for a stage that is
    skipped -- its fraction is 1.0 (or it keeps every one of the F features): threshold 1.0."""
    n, out = int(num_features), []
    for frac in (colsample_bytree, colsample_bylevel, colsample_bynode):
        if float(frac) >= 1.0:
            out.append(0)
            continue
        n = max(1, int(float(frac) * n))
        out.append(n if n < int(num_features) else 0)
    return tuple(out)


def _signed32(key: int) -> int:
    key &= 0xFFFFFFFF
    return key - (1 << 32) if key >= (1 << 31) else key


def column_thresholds(num_features: int, seed: int, tree_index: int, depth: int, nodes: list,
                      colsample_bytree: float = 1.0, colsample_bylevel: float = 1.0, colsample_bynode: float = 1.0,
                      dev="cpu") -> tuple:
    """(thr_tree, thr_level, thr_node [len(nodes)], eligible [len(nodes), F] bool) of the level at
    ``depth`` whose open nodes have the node-table ids ``nodes``: each stage's threshold is the
    k-th smallest priority (``feature_priority``: key = the stage's pseudo-node, or the node id)
    over the features that pass the stages before it; a feature may split node n iff its three
    priorities are <= the three thresholds. A skipped stage has threshold 1.0."""
    F = int(num_features)
    k_tree, k_level, k_node = column_counts(F, colsample_bytree, colsample_bylevel, colsample_bynode)
    fid = torch.arange(F, dtype=torch.int64, device=dev)
    ok = torch.ones(F, dtype=torch.bool, device=dev)
    thr_tree = thr_level = 1.0
    if k_tree:
        pr = _priorities(seed, tree_index, COL_TREE_KEY, fid)
        thr_tree = float(torch.kthvalue(pr, k_tree).values)
        ok &= pr <= thr_tree
    if k_level:
        pr = _priorities(seed, tree_index, COL_LEVEL_KEY - int(depth), fid)
        thr_level = float(torch.kthvalue(pr[ok], k_level).values)
        ok &= pr <= thr_level
    thr_node = torch.ones(len(nodes), dtype=torch.float64, device=dev)
    eligible = ok[None, :].repeat(len(nodes), 1)
    if k_node:
        for i, n in enumerate(nodes):
            pr = _priorities(seed, tree_index, int(n), fid)
            thr_node[i] = torch.kthvalue(pr[ok], k_node).values
            eligible[i] &= pr <= thr_node[i]
    return thr_tree, thr_level, thr_node, eligible
