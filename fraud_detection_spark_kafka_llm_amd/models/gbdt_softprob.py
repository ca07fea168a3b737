"""Multi-class gradient boosting, XGBoost-compatible (``multi:softprob``, hist).

Labels are integers ``0 .. C - 1`` with ``2 <= C <= 8``; the margins are ``C`` contiguous planes
``M[c][r]`` (``[C, N]`` fp64) that all start at ``base`` (``GBDTParams.base_score`` or 0.5: xgboost's
softmax objective takes the base score as the margin, untransformed). Round ``t``: one
``softprob_grad`` launch computes the ``2 C`` gradient planes from the round-start margins
(``csrc/softprob.h``: xgboost's ``SoftmaxMultiClassObj`` in fp64, weights folded in), then for
``c = 0 .. C - 1`` the grower grows tree ``t C + c`` from ``G[c]``, ``H[c]`` and its leaf values are
added to plane ``c`` alone. All ``C`` trees of a round see the same round-start probabilities, as in
xgboost; trees are stored in the order ``(t, c)``, so the class of tree ``i`` is ``i mod C``. Row and
column sampling key on the tree index ``t C + c``: each class tree draws its own sample.

The grower, the exact int64 histograms and the collectives are those of ``models/gbdt.py``: trees
are bitwise the same on host, device and every data-parallel world size. The gradients are external
to the grower here (its mode-0 route with ``g``, ``h`` supplied), so a tree runs the Python level
loop with a separate max |g|, |h| pass where a binary round runs the runner's fused prologue and
C++ level loop; ``bench/micro_softprob.py`` measures what that costs per tree.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from ..ops import native
from ..parallel.dist import Collectives
from ..utils import tracing
from .gbdt import GBDTParams, check_sampling
from .grower import GrowParams, Workspace, grow_tree
from .tree import prepare

DEFAULT_BASE_SCORE = 0.5


@dataclass
class GBDTSoftprobResult:
    trees: list                 # order (t, c): tree i belongs to class i % num_class
    num_class: int
    num_features: int
    base_margin: float
    params: GBDTParams
    train_seconds: float = 0.0
    shape: dict = field(default_factory=dict)
    margin: Optional[torch.Tensor] = None        # [C, N] training margins (return_margin=True)


def _host_array(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x if isinstance(x, np.ndarray) else list(x))


def check_labels(labels, max_classes: int) -> int:
    """The largest label of this rank's rows (-1 without rows); labels are integers in
    ``0 .. max_classes - 1``."""
    try:
        y = np.asarray(_host_array(labels), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"multi:softprob labels must be integers 0 .. C - 1: {e}") from None
    if y.size == 0:
        return -1
    if not np.all(np.isfinite(y)) or np.any(y != np.floor(y)) or y.min() < 0:
        raise ValueError("multi:softprob labels must be integers 0 .. C - 1")
    if y.max() >= max_classes:
        raise ValueError(f"multi:softprob supports at most {max_classes} classes, the labels reach {int(y.max())}")
    return int(y.max())


def check_weights(weights, n_rows: Optional[int] = None) -> Optional[np.ndarray]:
    if weights is None:
        return None
    w = np.asarray(_host_array(weights), dtype=np.float32).reshape(-1)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite and >= 0")
    if n_rows is not None and w.size != n_rows:
        raise ValueError(f"weights need one entry per row ({n_rows}), got {w.size}")
    return w


def fit_gbdt_softprob(features, labels, params: GBDTParams = GBDTParams(), device=None, weights=None,
                      num_class: Optional[int] = None, return_margin: bool = False, eval_set=None,
                      early_stopping_rounds=None, checkpoint=None, start_trees=None, checkpoint_dir=None,
                      resume: bool = False, eval_fn=None) -> GBDTSoftprobResult:
    """``num_class``: the class count ``C`` (default: the largest label + 1, at least 2; under an
    ambient process group the global largest, found with one MAX all-reduce per fit). Validation
    monitoring, early stopping, checkpoints and resume are not available on this route."""
    from ..ops.sparse import softprob_grad, softprob_limits
    from ..utils.config import default_device

    for name, v in (("eval_set", eval_set), ("early_stopping_rounds", early_stopping_rounds),
                    ("checkpoint", checkpoint), ("start_trees", start_trees), ("checkpoint_dir", checkpoint_dir),
                    ("resume", resume or None), ("eval_fn", eval_fn)):
        if v is not None:
            raise NotImplementedError(f"{name} is not supported by the multi:softprob trainer (validation "
                                      "monitoring, early stopping, checkpoints and resume are binary-only)")
    check_sampling(params)
    max_classes = int(softprob_limits()["max_classes"])
    if num_class is not None and (isinstance(num_class, bool) or int(num_class) != num_class
                                  or not 2 <= int(num_class) <= max_classes):
        raise ValueError(f"num_class must be an integer in 2 .. {max_classes}, got {num_class!r}")
    top = check_labels(labels, max_classes)
    w_host = check_weights(weights, len(labels) if hasattr(labels, "__len__") else None)
    coll = Collectives()
    dev = torch.device(device) if device is not None else default_device()
    if coll.active:
        top = int(coll.max(torch.tensor([top], dtype=torch.int64, device=dev))[0])
    C_ = max(top + 1, 2) if num_class is None else int(num_class)
    if C_ < top + 1:
        raise ValueError(f"num_class={C_} is below the largest label + 1 = {top + 1}")
    lib = native.lib()
    t0 = time.perf_counter()
    with tracing.span("gbdt.prepare"):
        Q, y, F, vc = prepare(features, labels, dev, params.max_bin, coll)
    dev = Q.device
    w = None if w_host is None else torch.from_numpy(w_host).to(dev)
    N = Q.n_rows
    base = DEFAULT_BASE_SCORE if params.base_score is None else float(params.base_score)
    margin = torch.full((C_, N), base, dtype=torch.float64, device=dev)
    G = torch.empty((C_, N), dtype=torch.float32, device=dev)
    H = torch.empty((C_, N), dtype=torch.float32, device=dev)
    gp = GrowParams(max_depth=params.max_depth, mode=0, lambda_=params.reg_lambda, min_child=params.min_child_weight,
                    min_gain=params.gamma, seed=params.seed, eta=params.learning_rate,
                    max_delta_step=params.max_delta_step, subsample=float(params.subsample),
                    colsample_bytree=float(params.colsample_bytree), colsample_bylevel=float(params.colsample_bylevel),
                    colsample_bynode=float(params.colsample_bynode))
    with tracing.span("gbdt.workspace"):
        ws = Workspace(Q)
    trees = []
    for t in range(params.n_estimators):
        with tracing.span("gbdt.round", round=t):
            # all C trees of the round see the round-start probabilities; the weights are in g, h
            softprob_grad(margin, y, w, G, H)
            for c in range(C_):
                tree = grow_tree(Q, ws, gp, t * C_ + c, g=G[c], h=H[c], coll=coll)
                node_value = torch.from_numpy(np.ascontiguousarray(tree.stats[:, 0])).to(dev)
                lib.tree_leaf_update(margin[c], ws.row_node, node_value)
                trees.append(tree.compacted())
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
        from .grower import dp_runner_stats

        dp_runner_stats()
    return GBDTSoftprobResult(trees, C_, F, base, params, time.perf_counter() - t0,
                              {"Fa": Q.Fa, "TB": Q.TB, "nnz": int(Q.csc_row.numel())},
                              margin if return_margin else None)
