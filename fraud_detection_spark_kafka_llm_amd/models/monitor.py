"""Validation monitoring of the GBDT trainer (models/gbdt.py): the validation margin, the
per-round metric and the early-stopping rule.

The validation rows never touch training: after a round's training-margin update the tree just
grown is added to the validation margin from the **device node table** (``tree_eval_update``, the
source ``leaf_update_stats_kernel`` reads), then the metric's integers are computed on the same
stream and copied to a pinned per-round slot with an event. Nothing here waits for the host, so
the deferred pipeline of ``fit_gbdt`` stays on; the host reads round t's slot after it has queued
round t + 1.

Contracts (csrc/eval.h): the margin after round t is bitwise ``base + sum_i score_csr(val,
[tree_i], cmp_less=True)`` added tree by tree; ``auc`` = U2 / (2 P N) and ``error`` are exact
integers, bitwise equal on host, device and every world size; ``logloss`` is an exact int64 sum of
``rint(w * l * 2^k)`` -- the same bits for any grid, thread count and world size on one backend,
while host and device may differ by the last bit of ``exp`` / ``log`` per term.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from ..ops import native

# metric -> is it maximised
METRICS = {"auc": True, "logloss": False, "error": False}


def eval_limits() -> dict:
    """Structural constants of the validation kernels: rows per workgroup and entries per
    wave-load of ``tree_eval_update``, the AUC tile, the reduction's block size."""
    return dict(native.lib().eval_limits())


def check_eval_args(eval_set, eval_metric, early_stopping_rounds) -> None:
    if eval_metric not in METRICS:
        raise ValueError(f"unknown eval_metric {eval_metric!r} (supported with a validation set: {sorted(METRICS)})")
    if len(eval_set) != 3:
        raise ValueError("eval_set = (features, labels, weights or None)")
    if eval_metric == "auc" and eval_set[2] is not None:
        raise NotImplementedError("weighted auc is not supported: use logloss / error with a weight column")
    if early_stopping_rounds is not None and int(early_stopping_rounds) < 1:
        raise ValueError("early_stopping_rounds must be >= 1")


class ValidationMonitor:
    def __init__(self, Q, ws, gp, coll, eval_set, metric: str, base: float, n_rounds: int,
                 early_stopping_rounds: Optional[int] = None):
        from ..ml.linalg import VectorColumn

        C = self.C = native.lib()
        dev = self.dev = Q.device
        self.Q, self.ws, self.gp, self.coll, self.metric = Q, ws, gp, coll, metric
        self.maximize = METRICS[metric]
        self.esr = None if early_stopping_rounds is None else int(early_stopping_rounds)
        vc, y, w = eval_set
        vc = vc if isinstance(vc, VectorColumn) else VectorColumn.from_rows(list(vc))
        if vc.size != Q.num_features:
            raise ValueError("validation and training features have different sizes")
        self.vc = vc.to(dev)
        indptr, idx, val = self.vc.csr()
        if val.dtype not in (torch.float32, torch.float64):
            val = val.to(torch.float64)
        self.csr = (indptr.to(torch.int64).contiguous(), idx.to(torch.int32).contiguous(), val.contiguous())
        n = self.n = len(self.vc)
        if not isinstance(y, torch.Tensor):
            y = torch.as_tensor(np.asarray(y, dtype=np.float32))
        self.y = y.to(device=dev, dtype=torch.float32).contiguous()
        self.w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.float32)).to(dev).contiguous()
        if self.y.numel() != n or (self.w is not None and self.w.numel() != n):
            raise ValueError("validation labels / weights and features have different row counts")
        # the global validation set: every rank holds its shard of the rows (collectives in program
        # order, here before the first tree's)
        self.dp = bool(coll.active and (coll.world > 1 or getattr(coll, "force", False)))
        wmax = float(self.w.max()) if (self.w is not None and n) else 1.0
        head = torch.tensor([n], dtype=torch.int64, device=dev)
        if self.dp:
            self.sizes = [int(v) for v in coll.all_gather(head).view(-1).tolist()]
            wmax = float(coll.max(torch.tensor([wmax], dtype=torch.float64, device=dev))[0])
        else:
            self.sizes = [n]
        self.n_global = sum(self.sizes)
        if self.n_global == 0:
            raise ValueError("the validation set is empty")
        self.k = int(C.eval_sum_kexp(self.n_global, wmax))
        if self.dp and metric == "auc":
            self.y_all = self._gather(self.y)        # labels do not change: gathered once
        self.margin = torch.full((n,), float(base), dtype=torch.float64, device=dev)
        thr = Q.thresholds
        thr = thr if isinstance(thr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64))
        self.quant = (Q.fid_orig.to(torch.int64).contiguous(), Q.boff.to(torch.int64).contiguous(),
                      thr.to(device=dev, dtype=torch.float64).contiguous())
        # per-round slots: the metric's three integers on the device, mirrored in pinned host memory
        self.slots = torch.zeros((max(n_rounds, 1), 3), dtype=torch.int64, device=dev)
        self.host = torch.zeros((max(n_rounds, 1), 3), dtype=torch.int64)
        self.events: dict = {}
        if dev.type == "cuda":
            self.host = self.host.pin_memory()
        self.history: list = []
        self.best_iteration = -1
        self.best_score = float("nan")

    # ------------------------------------------------------------------ the validation margin
    def add_device_tree(self) -> None:
        """The tree whose node table the level loop just finished (queued on the current stream,
        before the next tree's prologue overwrites the table)."""
        st, p = self.ws._levels, self.gp
        self.C.tree_eval_update(*self.csr, (st.feat, st.bin, st.left, st.right, st.leaf, st.stats, self.ws.kexp),
                                self.quant, float(p.eta), float(p.lambda_), float(p.max_delta_step), self.margin, 0)

    def add_tree(self, tree) -> None:
        """A host-built tree (trees deeper than the device level loop, and the replay of a
        checkpoint): the CSR scorer with the model's split test, one tree at a time."""
        from ..ml.tree_model import ensemble_arrays
        from ..ops.sparse import score_csr

        self.margin += score_csr(self.vc, ensemble_arrays([tree], "value", cmp_less=True))[:, 0]

    # ------------------------------------------------------------------ the metric
    def _gather(self, t: torch.Tensor) -> torch.Tensor:
        m = max(self.sizes)
        pad = torch.zeros(m, dtype=t.dtype, device=t.device)
        pad[: t.numel()] = t
        g = self.coll.all_gather(pad)
        return torch.cat([g[r, :s] for r, s in enumerate(self.sizes)]).contiguous()

    def queue(self, t: int) -> None:
        """Round t's metric integers -> slot t. Data parallel: issued through ``Collectives`` in
        program order, after the tree's last level collective and before the next tree's first --
        logloss / error sum their three int64 sums, auc all-gathers the margins and every rank
        sorts the whole set (redundant but exact: every rank computes identical bits)."""
        slot = self.slots[t]
        if self.metric == "auc":
            m, y = (self._gather(self.margin), self.y_all) if self.dp else (self.margin, self.y)
            self.C.eval_auc(m, y, slot)
        else:
            self.C.eval_sums(self.margin, self.y, self.w, self.k, slot, 0, 0)
            if self.dp:
                slot.copy_(self.coll.sum(slot))
        if self.dev.type == "cuda":
            self.host[t].copy_(slot, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            self.events[t] = ev
        else:
            self.host[t].copy_(slot)

    def read(self, t: int) -> bool:
        """Round t's metric into the history; True when early stopping ends the fit at t."""
        assert t == len(self.history)
        ev = self.events.pop(t, None)
        if ev is not None:
            ev.synchronize()
        a, b, c = (int(v) for v in self.host[t].tolist())
        if self.metric == "auc":
            v = float(a) / (2.0 * float(b) * float(c)) if b and c else float("nan")
        else:
            s = a if self.metric == "logloss" else b
            v = float(s) / float(c) if c else float("nan")
        if math.isnan(v):
            raise ValueError(f"validation {self.metric} is NaN: the validation set has one class (or no weight)")
        self.history.append(v)
        if self.best_iteration < 0 or (v > self.best_score if self.maximize else v < self.best_score):
            self.best_iteration, self.best_score = t, v          # (only a strict improvement)
        return self.esr is not None and t - self.best_iteration >= self.esr

    # ------------------------------------------------------------------ checkpoints
    def state(self) -> dict:
        return {"evals_result": {"validation": {self.metric: [float(v) for v in self.history]}},
                "best_iteration": int(self.best_iteration), "best_score": float(self.best_score)}

    def restore(self, st: dict, trees: list) -> None:
        hist = (st.get("evals_result") or {}).get("validation", {}).get(self.metric)
        if hist is None or "best_iteration" not in st or len(hist) != len(trees):
            raise RuntimeError("the checkpoint holds no validation history for this metric: it resumes only "
                               "without eval_set")
        for tr in trees:
            self.add_tree(tr)
        self.history = [float(v) for v in hist]
        self.best_iteration, self.best_score = int(st["best_iteration"]), float(st["best_score"])

    def evals_result(self) -> dict:
        return {"validation": {self.metric: list(self.history)}}
