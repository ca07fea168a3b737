"""Per-GPU micro-batch scorer with overlapped H2D / compute (C-03 consumer side).

Two HIP streams per device: ``h2d`` copies a pinned ring slot into one of ``depth`` device
buffers (SDMA engine), ``compute`` runs the fused featurize+score kernel on it, and the kernel
stores the fp64 scores and per-document status directly into page-locked host memory (zero-copy
over PCIe). A separate D2H copy would sit on the same SDMA queue behind the next batch's large
H2D and serialise the pipeline (measured: 2.6 -> 2.3 ms per 65536-dialogue step). Events chain
the stages, so with depth >= 2 the copy of batch i+1 runs underneath the kernel of batch i.
Device buffers are preallocated at the maximum micro-batch size: steady state allocates nothing.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..ops import native
from ..ops.text import (FLAG_IDF, FLAG_LR, FLAG_TREES, LONG_DOC_BYTES, PAD, STATUS_OK, ClassLinearScorer, FeatureSpec,
                        LinearScorer, PackedText, TreeArrays, _check_scorers, _flags, featurize_score)
from .ring import Slot


LONG_DOC_MIN = 4096      # raw bytes above which the streaming kernel defers to the long-dialogue kernel


def _split_scorer(scorer) -> tuple:
    """(lr, trees, classes): the scorer in the slot of its kind."""
    return (scorer if isinstance(scorer, LinearScorer) else None, scorer if isinstance(scorer, TreeArrays) else None,
            scorer if isinstance(scorer, ClassLinearScorer) else None)


def _score_width(scorer) -> int:
    """Scores per dialogue: the leaf width of a tree ensemble, the classes of a class scorer, else 1."""
    if isinstance(scorer, TreeArrays):
        return scorer.K
    return scorer.num_classes if isinstance(scorer, ClassLinearScorer) else 1


@dataclass
class _Stage:
    text: torch.Tensor
    offsets: torch.Tensor
    nnz: torch.Tensor
    ntok: torch.Tensor
    raw: torch.Tensor
    status: torch.Tensor
    h_raw: torch.Tensor
    h_status: torch.Tensor
    ev_h2d: torch.cuda.Event
    ev_compute: torch.cuda.Event
    ev_d2h: torch.cuda.Event
    long_host: torch.Tensor       # int32 pinned [max_docs]: indices of dialogues over LONG_DOC_MIN bytes
    long_dev: torch.Tensor        # its device copy (preallocated: no allocator traffic across streams)
    slot: Optional[Slot] = None
    very_long: Optional[tuple] = None   # (doc indices, raw [n, K]) of > 64 KB dialogues scored by segments
    n: int = 0


class GpuScorer:
    def __init__(self, spec: FeatureSpec, idf: Optional[np.ndarray], scorer, device, max_docs: int = 65536,
                 max_bytes: int = 256 << 20, depth: int = 2):
        if not isinstance(scorer, (LinearScorer, TreeArrays, ClassLinearScorer)):
            raise TypeError("scorer must be LinearScorer, TreeArrays or ClassLinearScorer")
        self.spec, self.scorer = spec, scorer
        self.dev = torch.device(device)
        self.C = native.lib()
        self.K = _score_width(scorer)
        self.idf = torch.as_tensor(np.asarray(idf, dtype=np.float64)).to(self.dev) if idf is not None else None
        lr, trees, classes = _split_scorer(scorer)
        _check_scorers(spec, lr, trees, classes)
        self.flags = _flags(spec, self.idf, lr, trees, want_csr=False, classes=classes)
        # class scores: W padded with rows of zeros up to the feature space, once
        self.cls = classes.tensors(self.dev, spec.dim) if classes is not None else (None, None)
        self.stop = spec.stop_table().tensors(self.dev) if spec.stop_table() else None
        self.vocab = spec.vocab_table().tensors(self.dev) if spec.vocab_table() else None
        self.lr_w = lr.weights(self.dev) if lr is not None else None
        self.tree_t = trees.tensors(self.dev) if trees is not None else None
        self.max_docs, self.max_bytes = max_docs, max_bytes
        self.h2d = torch.cuda.Stream(self.dev)
        self.compute = torch.cuda.Stream(self.dev)
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.dummy_i = torch.zeros(1, **i32)
        self.dummy_f = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.stages = []
        for _ in range(depth):
            self.stages.append(_Stage(
                torch.zeros(max_bytes + PAD, dtype=torch.uint8, device=self.dev),
                torch.zeros(max_docs + 1, dtype=torch.int64, device=self.dev),
                torch.zeros(max_docs, **i32), torch.zeros(max_docs, **i32),
                torch.zeros((max_docs, self.K), dtype=torch.float64, device=self.dev),
                torch.zeros(max_docs, **i32),
                torch.zeros((max_docs, self.K), dtype=torch.float64).pin_memory(),
                torch.zeros(max_docs, dtype=torch.int32).pin_memory(),
                torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event(),
                torch.zeros(max_docs, dtype=torch.int32).pin_memory(), torch.zeros(max_docs, **i32)))
        self._next = 0
        self._inflight: deque = deque()
        torch.cuda.synchronize(self.dev)

    # ------------------------------------------------------------------ pipeline
    def submit(self, slot: Slot) -> None:
        """Enqueue one slot. Blocks only if all ``depth`` stages are busy (waits the oldest)."""
        if slot.n_docs > self.max_docs or slot.n_bytes > self.max_bytes:
            raise ValueError("micro-batch exceeds the scorer's buffers")
        if len(self._inflight) == len(self.stages):
            raise RuntimeError("pipeline full: call collect() first")
        st = self.stages[self._next]
        self._next = (self._next + 1) % len(self.stages)
        n, nb = slot.n_docs, slot.n_bytes
        st.slot, st.n = slot, n
        long_idx = None
        n_long = 0
        very = None
        st.very_long = None
        if n:
            offs = slot.offsets[: n + 1].numpy()
            lens = offs[1:] - offs[:-1]
            if int(lens.max()) > LONG_DOC_MIN:
                sel = np.nonzero((lens > LONG_DOC_MIN) & (lens <= LONG_DOC_BYTES))[0]
                n_long = int(sel.size)
                very = np.nonzero(lens > LONG_DOC_BYTES)[0]
        # the stage's previous batch has fully drained (collect() synchronised on its event), so
        # its pinned index buffer may be rewritten here
        if n_long:
            st.long_host.numpy()[:n_long] = sel
            long_idx = st.long_dev[:n_long]
        with torch.cuda.stream(self.h2d):
            self.h2d.wait_event(st.ev_d2h)   # previous use of this stage fully drained
            st.text[: nb + PAD].copy_(slot.data[: nb + PAD], non_blocking=True)
            st.offsets[: n + 1].copy_(slot.offsets[: n + 1], non_blocking=True)
            if n_long:
                long_idx.copy_(st.long_host[:n_long], non_blocking=True)
            st.ev_h2d.record(self.h2d)
        with torch.cuda.stream(self.compute):
            self.compute.wait_event(st.ev_h2d)
            if n:
                # scores/status are stored by the kernel straight into pinned host memory: a D2H
                # copy would queue behind the next batch's 100+ MB H2D on the SDMA engine.
                args = (st.text[: nb + PAD], st.offsets[: n + 1], self.flags, self.spec.dim, self.stop, self.vocab,
                        float(self.spec.min_tf), self.idf, self.lr_w,
                        float(self.scorer.b) if self.lr_w is not None else 0.0, self.tree_t, self.K, self.dummy_i,
                        self.dummy_f, st.nnz, st.ntok, st.h_raw, st.h_status, None, 0)
                self.C.featurize_score(*args, None, *self.cls)
                if long_idx is not None:      # dialogues over 4 KB: long-dialogue kernel, same stream
                    self.C.featurize_score(*args, long_idx, *self.cls)
                if very is not None and very.size:    # over 64 KB: segmented device path (rare; syncs)
                    from ..ops.longdoc import featurize_long

                    lr, tr, classes = _split_scorer(self.scorer)
                    done, raw_l, *_ = featurize_long(st.text, slot.data.numpy(), offs, very, self.spec, self.idf, lr,
                                                     tr, self.dev, classes)
                    st.very_long = (very[done], raw_l.cpu().numpy())
            st.ev_compute.record(self.compute)
            st.ev_d2h = st.ev_compute
        self._inflight.append(st)

    def collect(self, copy: bool = True) -> tuple:
        """Wait for the oldest in-flight batch; returns (slot, raw scores [n, K] numpy).

        ``copy=False`` returns a view of the pinned result buffer, valid until this pipeline
        stage is reused (``depth`` submits later) — the zero-copy path of the streaming loop."""
        st = self._inflight.popleft()
        st.ev_d2h.synchronize()
        n = st.n
        raw = st.h_raw[:n].numpy()
        if copy:
            raw = raw.copy()
        status = st.h_status[:n].numpy()
        if st.very_long is not None and st.very_long[0].size:
            docs, vals = st.very_long
            raw = raw.copy() if not copy else raw
            raw[docs] = vals
            status = status.copy()
            status[docs] = STATUS_OK
        if n and np.any(status != STATUS_OK):
            bad = np.nonzero(status != STATUS_OK)[0]
            sub = PackedText.from_strings([bytes(st.slot.data[int(st.slot.offsets[i]):int(st.slot.offsets[i + 1])]
                                                 .numpy()).decode("utf-8", "replace") for i in bad])
            lr, tr, classes = _split_scorer(self.scorer)
            fix = featurize_score(sub, self.spec, idf=self.idf.cpu() if self.idf is not None else None, lr=lr,
                                  trees=tr, device="cpu", classes=classes)
            raw = raw.copy()
            raw[bad] = fix.raw.numpy()
        slot = st.slot
        st.slot = None
        return slot, raw

    @property
    def inflight(self) -> int:
        return len(self._inflight)

    def ready(self) -> bool:
        """True when the oldest in-flight batch has finished (collect() would not block)."""
        return bool(self._inflight) and self._inflight[0].ev_d2h.query()

    @property
    def depth(self) -> int:
        return len(self.stages)

    def score_packed(self, slot: Slot) -> np.ndarray:
        """Synchronous single batch (latency path)."""
        self.submit(slot)
        return self.collect()[1]


class HostScorer:
    """Same submit/collect interface on the host path (CPU-only deployments and tests)."""

    def __init__(self, spec: FeatureSpec, idf: Optional[np.ndarray], scorer, max_docs: int = 65536,
                 max_bytes: int = 256 << 20, depth: int = 1):
        self.spec, self.scorer = spec, scorer
        self.idf = torch.as_tensor(np.asarray(idf, dtype=np.float64)) if idf is not None else None
        self.max_docs, self.max_bytes = max_docs, max_bytes
        self._depth = max(1, depth)
        self._inflight: deque = deque()

    def submit(self, slot: Slot) -> None:
        if len(self._inflight) == self._depth:
            raise RuntimeError("pipeline full: call collect() first")
        n, nb = slot.n_docs, slot.n_bytes
        pt = PackedText(slot.data[: nb + PAD], slot.offsets[: n + 1].clone())
        lr, tr, classes = _split_scorer(self.scorer)
        res = featurize_score(pt, self.spec, idf=self.idf, lr=lr, trees=tr, device="cpu", classes=classes)
        self._inflight.append((slot, res.raw.numpy().copy()))

    def collect(self, copy: bool = True) -> tuple:
        return self._inflight.popleft()

    @property
    def inflight(self) -> int:
        return len(self._inflight)

    def ready(self) -> bool:
        return bool(self._inflight)

    @property
    def depth(self) -> int:
        return self._depth

    def score_packed(self, slot: Slot) -> np.ndarray:
        self.submit(slot)
        return self.collect()[1]


def make_scorer(spec: FeatureSpec, idf, scorer, device, max_docs: int = 65536, max_bytes: int = 256 << 20,
                depth: int = 2):
    device = torch.device(device)
    if device.type == "cuda":
        return GpuScorer(spec, idf, scorer, device, max_docs, max_bytes, depth)
    return HostScorer(spec, idf, scorer, max_docs, max_bytes, depth)


class MultiGpuScorer:
    """N per-device scorers behind the single-scorer interface (SURVEY PAR-06: partition
    consumers -> one pinned ring -> N GPU workers). Inference needs no collectives: micro-batches
    go round-robin to the devices and are collected in submission order, so downstream produce /
    commit order is the consume order. Each device keeps its own ``depth``-deep copy/compute
    pipeline, so up to ``sum(depth)`` micro-batches are in flight."""

    def __init__(self, scorers: list):
        if not scorers:
            raise ValueError("need at least one scorer")
        self.scorers = scorers
        self.max_docs = min(s.max_docs for s in scorers)
        self.max_bytes = min(s.max_bytes for s in scorers)
        self._order: deque = deque()
        self._rr = 0

    @property
    def depth(self) -> int:
        return sum(s.depth for s in self.scorers)

    @property
    def inflight(self) -> int:
        return len(self._order)

    def ready(self) -> bool:
        return bool(self._order) and self._order[0].ready()

    def submit(self, slot: Slot) -> None:
        for _ in range(len(self.scorers)):
            s = self.scorers[self._rr]
            self._rr = (self._rr + 1) % len(self.scorers)
            if s.inflight < s.depth:
                s.submit(slot)
                self._order.append(s)
                return
        raise RuntimeError("pipeline full: call collect() first")

    def collect(self, copy: bool = True) -> tuple:
        return self._order.popleft().collect(copy=copy)

    def score_packed(self, slot: Slot) -> np.ndarray:
        self.submit(slot)
        return self.collect()[1]


def make_multi_scorer(spec: FeatureSpec, idf, scorer, devices: list, max_docs: int = 65536,
                      max_bytes: int = 256 << 20, depth: int = 2):
    if len(devices) == 1:
        return make_scorer(spec, idf, scorer, devices[0], max_docs, max_bytes, depth)
    return MultiGpuScorer([make_scorer(spec, idf, scorer, d, max_docs, max_bytes, depth) for d in devices])
