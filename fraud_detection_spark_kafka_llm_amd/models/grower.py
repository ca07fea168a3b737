"""Level-wise histogram tree grower shared by DecisionTree, RandomForest and GBDT (X-09, X-10, X-13).

Per tree, ``tree_quant`` quantises the two row statistics (GBDT g*w, h*w; classification
w*[y==0], w*[y==1]) to integers q = rint(v * 2^k) (csrc/tree.h); the exponent k comes from the
global max |v| (all-reduced under data parallelism). Every histogram is then an exact int64 sum,
so trees are bitwise identical on the host, on the device and at any world size. A level (all its
nodes batched into every launch):
  1. histograms of the built nodes -- GBDT: the row-group engine (csrc/row_kernels.hip: row lists
     of the built rows, LDS int64 tables per bin group, the smaller sibling only); RF / DT: the CSC
     work items of the sampled features (csrc/tree_kernels.hip hist_lds_kernel, LDS atomics);
  2. data parallel: ONE reduce-scatter of the level's partials by feature shard (RCCL);
  3. split search over this rank's features (the larger sibling subtracted inside it), best
     split per node; data parallel: ONE all-gather of the per-shard best tuples;
  4. ``level_plan`` on the device: applies the splits to the device node table and plans the
     next level (open list, builds, subtraction rows; RF: the next level's feature sample and its
     active work items);
  5. partition of the rows to the children (zeroing the next level's histograms on the way).
The host reads a 16-byte count row per level and the node table once per tree. Drivers, fastest
first: the native runner's C++ level loops (csrc/bindings_level.cpp: RfLevels.gbdt_levels for GBDT
in one process and data parallel, RfBatch for RF trees in lockstep batches, models/forest_batch.py), the
Python device loop ``device_tree_steps`` (the test oracle of the native loops, and the CPU path
through the kernels' host twins), and the host loop ``grow_tree`` (deep trees). The data-parallel
machinery (level counters, LevelBatcher, feature shards, the runners' collectives) is in
models/dp_batch.py, the host-side trees (GrowParams, TreeTable, tree_from_host) in
models/tree_table.py; both are re-exported here.

``device_tree_steps`` resolves once how a tree runs (``_resolve_tree`` -> ``_Path`` with one
``_Driver``) and holds only the control flow and the yields; its stages (prologues, ``_open_level``,
``_level_sample``, ``_hist_out``, ``_level_hist``, ``_level_rows``, ``_split_search``, the two
``_*_plan_partition``, ``_read_tree``) are module-level helpers that read that record. (A table of
mix64(feature) for the RF sampler was tried and removed: profiles/r6/rf_dp_busy_fmix_REJECTED.txt.)
"""
from __future__ import annotations

import enum
import functools
import os
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from ..ml.tree_model import Tree
from ..ops import native
from ..utils import tracing
from . import quantize as qmod
from .dp_batch import (LEVEL_STATS, LEVEL_TIMING, CollStep, FeatureShards, LaneBufs, LevelBatcher,  # noqa: F401
                       _CollTimer, _DP_RUNNERS, _DpCollectives, _Lane, _level_collective_ms, _rccl_comm, drive,
                       dp_runner_stats, level_collective_ms, reset_level_stats)
from .quantize import Quantized
from .tree_table import GrowParams, PendingTree, TreeTable, _impurity, leaf_values_device, tree_from_host  # noqa: F401

NEG_INF = float("-inf")
MAX_CT = 8                      # column tiles per pass (csrc/tree_kernels.hip launch_hist)
# rows per wave of the dense hot-feature histogram kernel (fixed: shorter ranges for launches with
# few feature groups measured no better, profiles/r2_gbdt_knob_sweep.txt)
DENSE_RANGE_ROWS = 32768
# levels 0..DENSE_MAX_DEPTH build the hot features' histograms with the dense kernel (every row
# streamed, slot-masked); deeper levels use their CSC items (only live entries multiplied)
DENSE_MAX_DEPTH = 2
# histogram launches of one pass (CSC groups, dense groups) run concurrently on this many HIP
# streams: they add into disjoint feature ranges with integer atomics, so the order is free and
# the kernels fill each other's tails
HIST_STREAMS = 4


# row-group histogram engine (models/quantize.RowGroups, csrc/row_kernels.hip): every level's
# histograms from the row-group CSR of the built rows, in place of the CSC / dense passes
ROWHIST = True
RG_DBG = 0   # diagnostics only (csrc/tree.h RgHistArgs::dbg)
# RF passes over sampled features (class counts, np = 1) read a packed row state (slot + class
# counts in one word per row) and a device-compacted list of the active work items
# (tree_hist_sampled); with at most this many open nodes the list is compacted by the pass itself
LISTED_MAX_NODES = 2
# RF levels >= 1 launch one wave per active work item from lists compacted with the previous
# level's plan (0: the r4 passes, a wave per item slot or a fixed listed grid), on shards of any
# size: once the packed items skip their unsampled features and the selects of a level are one
# launch, the listed passes win at 1.25M rows too (DP=8 shard, forced collectives: 0.456 -> 0.446 s
# a forest, profiles/r5/rf_lean_presel_ab_1M.jsonl; before, 143 -> 207 us a pass the other way); at
# 10M rows they win (0.768 -> 0.747 s)
PRESELECT = True
# RF levels >= 1 read the packed row state (slot | class-count digits) written by the previous
# level's partition instead of a row pass of their own (slot pack / masked digits: ~87 us per level
# at 10M rows, 173 ms of a 500-tree forest's kernel time, profiles/r5/NOTES.md)
FUSED_PACK = True
# device levels issue their kernels through the native per-level runner (csrc/bindings_level.cpp
# RfLevels: hist / split / plan / partition, one host call each) instead of ~20 Python-level calls:
# _Path.runner, and in one process the fused prologue (_Driver.RUNNER; 0: _Driver.PYTHON)
NATIVE_LEVELS = True
# the partition's row pass writes the next level's row-list counts (runner levels, <= 4M rows)
PARTITION_COUNTS = True
# row-group passes reduce per-workgroup partial tables (0: every workgroup's atomics); in the
# listed passes over several slots a workgroup whose chunk straddles a slot boundary still
# flushes with atomics
RG_PARTIALS = True
# GBDT trees on the row-group engine, one process or data parallel: the level loop runs in the
# runner (C++, RfLevels.gbdt_levels: _Driver.CXX_GBDT; 0: the generic loop of device_tree_steps)
GBDT_CXX_LEVELS = True
# ... which, in one process, builds the sibling with fewer rows (not the smaller hessian sum) where
# the row lists count their own rows (above 4M rows, or PARTITION_COUNTS off): same trees, shorter
# lists; the partition's rows per node, kept per 512-row wave, also stand in for the lists'
# counting pass
GBDT_CHOOSE_ROWS = True
# RF / DT count passes: the LDS-atomic kernel (one ds_add_u64 per entry) instead of i8 MFMA
RF_LDS = True
# RF levels under data parallelism reduce-scatter only the bins of the level's sampled features
# (FeatureShards.sample_compact). "auto": when the reduce-scatter crosses ranks (world > 1; at
# world 1 it is a local copy and the layout pass only costs); "1" always (the world-1 RCCL
# rehearsal of the path); "0" never
RF_COMPACT = os.environ.get("FDX_RF_COMPACT", "auto")


# GBDT trees grow with the device-resident level loop (grow_tree_device): split application and
# next-level planning run on the GPU, the host reads 16 bytes per level and the node table once
# per tree (FDX_DEVICE_LEVELS=0: host loop)
DEVICE_LEVELS = True
PARTITION_WPS = 256  # blocks per column split (device partition)
# debug: check on the host that every open node of a data-parallel level is built or subtracted
# (its histogram row is then written before the split search reads it; _dp_level_rows)
LEVEL_CHECKS = os.environ.get("FDX_LEVEL_CHECKS", "0") == "1"


class Workspace:
    """Per-engine device buffers reused across trees (digits, slot table, row -> node map)."""

    def __init__(self, Q: Quantized, max_nodes_per_level: int = 0):
        dev = Q.device
        self.rowdig = torch.empty((Q.n_rows, 2), dtype=torch.int32, device=dev)
        self.kexp = torch.zeros(2, dtype=torch.int32, device=dev)
        self.totals = torch.zeros(2, dtype=torch.int64, device=dev)
        self.maxabs = torch.zeros(2, dtype=torch.float64, device=dev)
        # padded to a multiple of 64 rows for the dense kernel (pad bytes stay 0xff = no slot)
        self.slot8_pad = torch.full((Q.n_pad,), 0xFF, dtype=torch.uint8, device=dev)
        self.slot8 = self.slot8_pad[:Q.n_rows]
        self.digp = torch.zeros((8, Q.n_pad), dtype=torch.uint8, device=dev) if Q.dense is not None else None
        self._dense_groups: dict = {}
        self.dense_waves = int(native.lib().tree_dense_waves())
        self.row_node = torch.zeros(Q.n_rows, dtype=torch.int32, device=dev)
        self.Fa = Q.Fa
        self.dev = dev
        self.Q = Q
        self._shards = None
        self.staging = Staging(dev)
        self._streams = None
        self.split_cache: dict = {}          # _best_splits scratch per level shape

    def rowgroups(self):
        """The row-group CSR when the row-group engine is on and covers every feature (else None),
        plus the level's row-list buffers."""
        if not ROWHIST:
            return None
        rg = self.Q.rowgroups()
        if not rg.complete:
            return None
        if getattr(self, "rg_list", None) is None:
            self.rg_list = torch.empty(self.Q.n_rows, dtype=torch.int32, device=self.dev)
            self.rg_start = torch.zeros(66, dtype=torch.int32, device=self.dev)
            nw = -(-self.Q.n_rows // native.lib().tree_rg_list_rows(self.Q.n_rows))   # waves of the list kernels
            self.rg_work = torch.zeros(64 * (2 + nw), dtype=torch.int32, device=self.dev)
            self.rg_listdig = torch.empty((self.Q.n_rows, 2), dtype=torch.int32, device=self.dev)
        return rg

    def keepbits(self, params) -> Optional[torch.Tensor]:
        """[ceil(N / 64)] int64: one keep bit per row of a subsampled GBDT round, written by the
        quantisation (a ballot per 64 rows) and read by the row lists (None without subsampling)."""
        if params.mode != 0 or params.subsample >= 1.0:
            return None
        if getattr(self, "_keepbits", None) is None:
            self._keepbits = torch.zeros((self.Q.n_rows + 63) // 64, dtype=torch.int64, device=self.dev)
        return self._keepbits

    def rg_emdig(self) -> torch.Tensor:
        """[N, 2] digit words zeroed outside the one built node (entry-major listed pass)."""
        if getattr(self, "_rg_emdig", None) is None:
            self._rg_emdig = torch.empty((self.Q.n_rows, 2), dtype=torch.int32, device=self.dev)
        return self._rg_emdig

    def rg_part(self, rg, other_work=None) -> torch.Tensor:
        """[n_wg, gbins, 2] int64 scratch of a row-group pass's partial tables (sized for the
        larger of rg.work() and ``other_work``)."""
        n_wg = max(int(rg.work().shape[1]), int(other_work.shape[1]) if other_work is not None else 0)
        need = n_wg * int(rg.gbin.shape[1]) * 2
        t = getattr(self, "_rg_part", None)
        if t is None or t.numel() < need:
            t = self._rg_part = torch.empty(need, dtype=torch.int64, device=self.dev)
        return t

    def dig16(self) -> torch.Tensor:
        """[N] int16: the rows' two class-count digits (RF), written by the runner's quantisation
        for the fused partition's packed row state (2 bytes a row instead of the 8-byte word)."""
        if getattr(self, "_dig16", None) is None:
            self._dig16 = torch.empty(self.Q.n_rows + 8, dtype=torch.int16, device=self.dev)
        return self._dig16

    def rowpack(self) -> torch.Tensor:
        """[N] int32 packed row state of the sampled (RF) passes: slot | class-count digits << 8."""
        if getattr(self, "_rowpack", None) is None:
            self._rowpack = torch.empty(self.Q.n_rows, dtype=torch.int32, device=self.dev)
        return self._rowpack

    def item_list(self, gi: int, grp) -> tuple:
        """(list, count) device scratch of a listed pass over item group ``gi`` (one per group: the
        groups' passes run on concurrent streams)."""
        lists = getattr(self, "_item_lists", None)
        if lists is None:
            lists = self._item_lists = {}
        slots = grp.wave_order().numel()
        need = 8 * ((-(-slots // 4) + 7) // 8 * 4)          # per-XCD lists (tree_kernels.hip hist_select)
        cur = lists.get(gi)
        if cur is None or cur[0].numel() < need:
            cur = lists[gi] = (torch.empty(need, dtype=torch.int32, device=self.dev),
                               torch.zeros(8, dtype=torch.int32, device=self.dev))
        return cur

    def run_concurrent(self, launches: list) -> None:
        """Run the launches on HIST_STREAMS side streams joined back into the current stream
        (serially on the current stream on the host or with one stream). The first launch (the
        long cold-feature CSC pass) runs on the current stream and the others share the
        HIST_STREAMS - 1 side streams, so none queues behind it (a short launch behind it added
        0.15-0.25 ms to every level)."""
        nstreams = getattr(self, "hist_streams", HIST_STREAMS)
        if self.dev.type != "cuda" or nstreams <= 1 or len(launches) <= 1:
            for fn in launches:
                fn()
            return
        if self._streams is None:
            self._streams = [torch.cuda.Stream(self.dev) for _ in range(nstreams - 1)]
        main = torch.cuda.current_stream(self.dev)
        start = main.record_event()
        ns = len(self._streams)
        # the long first launch stays on the current stream and is issued first: it starts right
        # behind the slot pass and the next level's kernels follow it in stream order, with no
        # cross-stream event wait on the critical path (~15 + ~35 us per level measured on the
        # side-stream variant); the side streams wait for ``start``, recorded before it
        launches[0]()
        for i, fn in enumerate(launches[1:]):
            s = self._streams[i % ns]
            s.wait_event(start)
            with torch.cuda.stream(s):
                fn()
        for s in self._streams[:min(len(launches) - 1, ns)]:
            main.wait_stream(s)

    def dense_groups(self, bt: int, fg: int):
        """(gfid, gdense) device arrays [ngroups * fg] of the hot features with ``bt`` row tiles,
        -1 padded; cached."""
        key = (bt, fg)
        if key in self._dense_groups:
            return self._dense_groups[key]
        Q = self.Q
        d = np.nonzero(Q.hot_bt == bt)[0]
        per_wg = fg * self.dense_waves
        ng = (d.size + per_wg - 1) // per_wg * self.dense_waves
        gfid = np.full(ng * fg, -1, dtype=np.int32)
        gden = np.zeros(ng * fg, dtype=np.int32)
        gfid[:d.size] = Q.hot[d]
        gden[:d.size] = d
        out = self._dense_groups[key] = (torch.from_numpy(gfid).to(self.dev), torch.from_numpy(gden).to(self.dev))
        return out

    def gh(self) -> tuple:
        """[N] float32 g, h buffers of the GBDT rounds (computed on the device per round)."""
        if getattr(self, "_gh", None) is None:
            self._gh = (torch.empty(self.Q.n_rows, dtype=torch.float32, device=self.dev),
                        torch.empty(self.Q.n_rows, dtype=torch.float32, device=self.dev))
        return self._gh

    def iota(self, n: int) -> torch.Tensor:
        """[0, 1, ..., n - 1] int32 on the device (cached: one allocation per workspace)."""
        t = getattr(self, "_iota", None)
        if t is None or t.numel() < n:
            t = self._iota = torch.arange(max(n, 64), dtype=torch.int32, device=self.dev)
        return t[:n]

    def shards(self, coll) -> "FeatureShards":
        if getattr(self, "_shards", None) is None or self._shards.S != coll.world:
            self._shards = FeatureShards(self.Q, coll.world, coll.rank)
        return self._shards


class Staging:
    """Per-level small host arrays (slot maps, subtraction triples, node totals, partition lists)
    gathered into one pinned buffer and sent with ONE async H2D copy, instead of a synchronous
    pageable copy per array (~15 per level, the bulk of the grower's host overhead). Two pinned
    buffers alternate; an event guards reuse. Tensors returned by ``upload`` are views into a
    device buffer that the next upload overwrites in stream order, so callers consume them before
    uploading again (the grower uploads at level start and after the split decisions)."""

    def __init__(self, dev: torch.device, cap: int = 1 << 16):
        self.dev = dev
        self.cuda = dev.type == "cuda"
        self._cap = 0
        self._host, self._events, self._flip = [None, None], [None, None], 0
        self._reserve(cap)
        self._items: list = []
        self._off = 0

    def _reserve(self, cap: int) -> None:
        if cap <= self._cap:
            return
        if self.cuda:
            torch.cuda.synchronize(self.dev)
        self._cap = cap
        mk = (lambda: torch.empty(cap, dtype=torch.uint8).pin_memory()) if self.cuda else \
            (lambda: torch.empty(cap, dtype=torch.uint8))
        self._host = [mk(), mk()]
        self._events = [None, None]
        self._dev = torch.empty(cap, dtype=torch.uint8, device=self.dev)

    def add(self, arr) -> int:
        a = np.ascontiguousarray(arr)
        self._items.append(a)
        return len(self._items) - 1

    def upload(self) -> list:
        offs, total = [], 0
        for a in self._items:
            total = (total + 7) & ~7
            offs.append(total)
            total += a.nbytes
        if total > self._cap:
            self._reserve(max(total, 2 * self._cap))
        k = self._flip
        self._flip ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        host = self._host[k].numpy()
        for a, o in zip(self._items, offs):
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        if self.cuda:
            self._dev[:total].copy_(self._host[k][:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._events[k] = ev
            src = self._dev
        else:
            src = self._host[k].clone()
        out = []
        for a, o in zip(self._items, offs):
            t = src[o:o + a.nbytes].view(_TORCH_DTYPE[a.dtype.str[1:]]).view(a.shape)
            out.append(t)
        self._items = []
        return out


_TORCH_DTYPE = {"i4": torch.int32, "i8": torch.int64, "f8": torch.float64, "f4": torch.float32}


def slots_per_tile(np_: int) -> int:
    """Node slots per 16-column MFMA tile: 2 statistics x ``np_`` digit planes per slot."""
    return 16 // (2 * np_)


def pass_ct(np_: int, cnt: int) -> int:
    """Column tiles (power of two) for ``cnt`` node slots."""
    per = slots_per_tile(np_)
    ct = 1
    while ct * per < cnt:
        ct *= 2
    return ct


class ColumnSampler:
    """GBDT column sampling of one workspace (models/rf_sampling.column_thresholds is its oracle):
    the stage counts, the device thresholds of the tree stage [1], of every level's stage [D] and of
    a level's open nodes [2^D], the pseudo-node keys, and the [D, F] byte mask of the tree and level
    stages that the node-stage searches and the split search read (one byte per feature index,
    written once per tree). The native runner fills and reads the tensors itself
    (RfLevels.col_begin / col_level); ``begin`` / ``level_args`` are the same launches for the
    Python loops (device or host twins). Nothing is allocated unless a fraction is < 1."""

    @classmethod
    def of(cls, Q: Quantized, ws: "Workspace", params: GrowParams) -> Optional["ColumnSampler"]:
        fr = (params.colsample_bytree, params.colsample_bylevel, params.colsample_bynode)
        if params.mode != 0 or all(f >= 1.0 for f in fr):
            return None
        key = (fr, params.max_depth)
        cur = getattr(ws, "_col", None)
        if cur is None or cur.key != key:
            cur = ws._col = cls(Q, params, key)
        return cur if cur.on else None

    def __init__(self, Q: Quantized, params: GrowParams, key):
        from . import rf_sampling

        dev, D = Q.device, max(int(params.max_depth), 1)
        self.key, self.F, self.D = key, int(Q.num_features), D
        self.ks = rf_sampling.column_counts(self.F, *key[0])
        self.on = any(self.ks)
        f64 = lambda n: torch.ones(n, dtype=torch.float64, device=dev)   # noqa: E731
        self.tree, self.level, self.node = f64(1), f64(D), f64(2 ** D)
        self.tkey = torch.tensor([-1], dtype=torch.int32, device=dev)          # 0xFFFFFFFF
        self.lkeys = torch.tensor([-2 - d for d in range(D)], dtype=torch.int32, device=dev)   # 0xFFFFFFFE - d
        outer = bool(self.ks[0] or self.ks[1])
        self.mask = torch.empty((D, self.F), dtype=torch.uint8, device=dev) if outer else None
        # features that pass the tree stage / the tree and level stages (the searches' populations)
        self.pop1 = self.ks[0] or self.F
        self.pop2 = self.ks[1] or self.pop1

    def nbytes(self) -> int:
        return int(self.mask.numel()) if self.mask is not None else 0

    def runner_cfg(self) -> dict:
        return dict(col_k=list(self.ks), col_tree=self.tree, col_level=self.level, col_node=self.node,
                    col_tkey=self.tkey, col_lkeys=self.lkeys, col_mask=self.mask)

    def begin(self, C, seed: int, tree: int) -> None:
        if self.mask is None:
            return
        t = self.tree if self.ks[0] else None
        if self.ks[0]:
            C.tree_col_thresholds(seed, tree, self.tkey, True, self.F, self.ks[0], self.tree, pop=self.F)
        if self.ks[0] and self.ks[1]:      # row 0 = the tree stage alone, for the level searches
            C.tree_col_mask(seed, tree, t, None, self.mask[:1])
        if self.ks[1]:
            C.tree_col_thresholds(seed, tree, self.lkeys, True, self.F, self.ks[1], self.level,
                                  outer_mask=self.mask[0] if self.ks[0] else None, pop=self.pop1)
        C.tree_col_mask(seed, tree, t, self.level if self.ks[1] else None, self.mask)

    def level_args(self, C, seed: int, tree: int, d: int, open_ids: torch.Tensor) -> tuple:
        """(node-stage thresholds of the open nodes or None, tree_split_find's column arguments)."""
        thr = None
        if self.ks[2]:
            thr = self.node[:open_ids.numel()]
            C.tree_col_thresholds(seed, tree, open_ids, False, self.F, self.ks[2], thr,
                                  outer_mask=self.mask[d] if self.mask is not None else None, pop=self.pop2)
        return thr, (dict(col_mask=self.mask[d]) if self.mask is not None else {})


def _best_splits(C, hist, totals, boff, nbins, zbin, fid_orig, node_ids, kexp, params, feat_thr, tree_index, Fa,
                 f0, node_tree=None, cache: Optional[dict] = None, out: Optional[torch.Tensor] = None,
                 row_of: Optional[torch.Tensor] = None, **col_kw):
    """Per node: (gain float64, feature (+f0) int64, bin int64, left sums int64 [2]) of the best
    split over Fa features of ``hist`` [nodes, boff[Fa], 2]; gain -inf without a valid candidate.
    Returned as one int64 tensor [nodes, 5] (gain bit-cast) for a single device->host copy.
    ``cache`` (a workspace dict): the per-(node, feature) scratch is allocated once per level
    shape and reused (stream order: the previous level's split kernels are done with it).
    ``out``: write the tuples there (a tree's rows of a batched all-gather). ``row_of``: the
    histogram row of each node (data-parallel levels; default row = node index). (The kernels
    take the row stride from hist.size(1), never from boff[Fa]: a compact RF level's boff[Fa]
    is the next shard's first offset, not this shard's end.)"""
    dev = hist.device
    nl = int(node_ids.numel())
    if Fa == 0:
        if out is None:
            out = torch.empty((nl, 5), dtype=torch.int64, device=dev)
        out.zero_()
        out[:, 0] = torch.tensor(NEG_INF, dtype=torch.float64).view(torch.int64)
        out[:, 1:3] = -1
        return out
    bufs = cache.get((nl, Fa)) if cache is not None else None
    if bufs is None:
        bufs = (torch.empty((nl, Fa), dtype=torch.float64, device=dev), torch.empty((nl, Fa), dtype=torch.int32, device=dev),
                torch.empty((nl, Fa, 2), dtype=torch.int64, device=dev))
        if cache is not None:
            cache[(nl, Fa)] = bufs
    out_gain, out_bin, out_left = bufs
    # features with > 16 bins get a wave each (tree_kernels.hip split_wide_kernel): listed once per
    # nbins tensor (kept on the tensor itself, shared by every forest lane; one read of the counts)
    wide = _wide_features(nbins, Fa) if dev.type == "cuda" else None
    C.tree_split_find(hist, totals, boff, nbins, zbin, fid_orig, node_ids, kexp, int(params.mode),
                      float(params.lambda_), float(params.min_child), feat_thr, int(params.seed), int(tree_index),
                      out_gain, out_bin, out_left, node_tree, wide, row_of, **col_kw)
    # best gain per node, ties to the lowest feature index (deterministic whatever the batch shape):
    # one native reduction instead of ~9 small torch launches per level
    if out is None:
        out = torch.empty((nl, 5), dtype=torch.int64, device=dev)
    if nl:
        C.tree_split_best(out_gain, out_bin, out_left, int(f0), out)
    return out


def _choose_np(params: GrowParams, weight) -> int:
    """Digit planes per statistic: integer class counts (Poisson(1) <= 32, no instance weights)
    fit one signed byte; everything else uses 4 planes (30-bit fixed point)."""
    return 1 if (params.mode != 0 and weight is None) else 4


def grow_tree(Q: Quantized, ws: Workspace, params: GrowParams, tree_index: int,
              g: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None,
              label: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
              bootstrap: bool = False, coll=None, deferred: bool = False, on_first_wait=None,
              margin: Optional[torch.Tensor] = None):
    """``coll`` (parallel.dist.Collectives): data-parallel level with feature-sharded split
    finding when world > 1 -- partial histograms are reduce-scattered by feature shard, every
    rank searches splits of its own shard, and the per-node best tuples are all-gathered
    (SURVEY PAR-02). ``coll.force`` runs the same collective path at world size 1 (RCCL check)."""
    C = native.lib()
    use_coll = coll is not None and coll.active
    shards = ws.shards(coll) if use_coll and (coll.world > 1 or getattr(coll, "force", False)) else None
    if device_levels_ok(params, weight):
        return grow_tree_device(Q, ws, params, tree_index, g, h, weight, coll if use_coll else None, shards,
                                label=label, bootstrap=bootstrap, deferred=deferred, on_first_wait=on_first_wait,
                                margin=margin)
    if margin is not None and g is None:           # (GBDT: this round's gradients)
        g, h = ws.gh()
        C.tree_logistic_grad(margin, label, weight, g, h)
    if on_first_wait is not None:
        on_first_wait()
    dev = Q.device
    np_ = _choose_np(params, weight)
    spt = slots_per_tile(np_)
    pass_slots = spt * MAX_CT
    max_nodes = 2 ** (params.max_depth + 1)
    # host node table

    ws.row_node.zero_()
    with tracing.span("tree.quant"):
        _quantise(C, Q, ws, params, tree_index, _TreeInput(g, h, label, weight, bootstrap, margin), np_,
                  coll if use_coll else None)
    tot = coll.sum(ws.totals) if use_coll else ws.totals
    head = torch.cat([tot, ws.kexp.to(torch.int64)]).cpu().numpy()
    tab = TreeTable(head[:2].astype(np.int64))
    parent, left, right, stats, is_leaf = tab.parent, tab.left, tab.right, tab.stats, tab.is_leaf
    kexp = head[2:4].astype(np.int64)
    scale = np.ldexp(1.0, -kexp)                    # value of one quantisation step per statistic
    level = [0]
    prev_hist = None
    prev_index: dict = {}
    TB = Q.TB
    feat_thr_all = None
    col = ColumnSampler.of(Q, ws, params)
    if col is not None:
        col.begin(C, int(params.seed), int(tree_index))

    for d in range(params.max_depth + 1):
        open_nodes = [n for n in level if not is_leaf[n]]
        if d == params.max_depth or not open_nodes:
            for n in open_nodes:
                is_leaf[n] = True
            break
        # --- decide which nodes to build (smaller sibling) and which to subtract
        build, subtract = [], []
        if d == 0 or params.feat_k:
            # RF: a feature sampled at this level may not have been built for the parent, so
            # sibling subtraction would read a missing parent histogram: build every open node
            build = list(open_nodes)
        else:
            seen = set()
            for n in open_nodes:
                p = parent[n]
                if p in seen:
                    continue
                seen.add(p)
                a, b = left[p], right[p]
                a_open, b_open = not is_leaf[a], not is_leaf[b]
                if a_open and b_open:
                    wa = _weight(stats[a], params.mode)
                    wb = _weight(stats[b], params.mode)
                    small, large = (a, b) if wa <= wb else (b, a)
                    build.append(small)
                    subtract.append((large, p, small))
                elif a_open:
                    build.append(a)
                elif b_open:
                    build.append(b)
        local = {n: i for i, n in enumerate(open_nodes)}
        nl = len(open_nodes)
        nb = len(build)
        if shards is None:
            cur_hist = torch.zeros((nl, TB, 2), dtype=torch.int64, device=dev)
            hist_target, target_of, h_boff, h_stride = cur_hist, local, Q.boff, TB
        else:
            # local partials of the built nodes, shard-major (reduce-scattered as they stand)
            rs_buf = shards.target(nb, dev)
            hist_target = rs_buf.view(shards.S * nb, shards.Bs, 2)
            target_of = {n: k for k, n in enumerate(build)}
            h_boff, h_stride = shards.boff_packed(nb), shards.Bs
        # --- small per-level arrays, one staged upload
        stg = ws.staging
        h_ns = None
        if d > 0:
            ns = np.full(max_nodes, -1, dtype=np.int32)
            ns[np.asarray(build, dtype=np.int64)] = np.arange(nb, dtype=np.int32)
            h_ns = stg.add(ns)
        passes = []
        for s0 in range(0, nb, pass_slots):
            cnt = min(pass_slots, nb - s0)
            s2n = np.array([target_of[build[s0 + k]] for k in range(cnt)], dtype=np.int32)
            passes.append((s0, cnt, stg.add(s2n)))
        h_sub = None
        if subtract:
            h_sub = (stg.add(np.array([local[a] for a, _, _ in subtract], dtype=np.int32)),
                     stg.add(np.array([prev_index[p] for _, p, _ in subtract], dtype=np.int32)),
                     stg.add(np.array([local[s] for _, _, s in subtract], dtype=np.int32)))
        h_tot = stg.add(np.stack([stats[n] for n in open_nodes]).astype(np.int64))
        h_ids = stg.add(np.array(open_nodes, dtype=np.int32))
        h_bidx = stg.add(np.array([local[n] for n in build], dtype=np.int64))
        up = stg.upload()
        node_slot = up[h_ns] if h_ns is not None else None
        # RF: exact k-of-F feature sample per open node (k-th smallest priority, on device) and
        # the level's union mask; histogram items without a sampled feature are skipped
        feat_thr = feat_mask = None
        if params.feat_k:
            feat_thr = torch.empty(nl, dtype=torch.float64, device=dev)
            feat_mask = torch.empty(Q.Fa, dtype=torch.uint8, device=dev)
            C.tree_rf_sample(int(params.seed), int(tree_index), up[h_ids], int(Q.num_features), int(params.feat_k),
                             Q.fid_orig, feat_thr, feat_mask, None)
        # --- histograms, up to `pass_slots` node slots per pass
        with tracing.span("tree.hist"):
            # RF levels read only the sampled features' CSC items (the dense block would stream
            # every hot feature for a handful of sampled ones)
            use_dense = Q.dense is not None and d <= DENSE_MAX_DEPTH and not params.feat_k
            for s0, cnt, h_s2n in passes:
                slot8 = None
                if d > 0:
                    C.tree_slot8(ws.row_node, node_slot, s0, cnt, ws.slot8, None, None)
                    slot8 = ws.slot8
                ws.run_concurrent(_csc_dense_launches(
                    C, Q, ws, np_, cnt, d == 0, use_dense, _RowState(slot8, ws.rowdig, None), feat_mask,
                    _HistOut(hist_target, h_boff, h_stride, up[h_s2n])))
        totals, node_ids = up[h_tot], up[h_ids]
        col_kw = {}
        if col is not None:         # (the node stage rides in feat_thr, as RF's per-node sample does)
            feat_thr, col_kw = col.level_args(C, int(params.seed), int(tree_index), d, node_ids)
        sub_t = tuple(up[h] for h in h_sub) if h_sub is not None else None
        if shards is None:
            if sub_t is not None:
                C.tree_hist_subtract(prev_hist, cur_hist, *sub_t, TB)
            with tracing.span("tree.split"):
                packed = _best_splits(C, cur_hist, totals, Q.boff, Q.nbins, Q.zbin, Q.fid_orig, node_ids, ws.kexp,
                                      params, feat_thr, tree_index, Q.Fa, 0, **col_kw)
                packed = packed.cpu().numpy()
        else:
            with tracing.span("tree.reduce_scatter"), _CollTimer(dev):
                # rows keep the shard-major stride Bs (>= this shard's bins): the split search
                # reads them in place; every open node is built or subtracted, so no zero fill
                mine = coll.reduce_scatter(rs_buf) if nb else None            # [nb, Bs, 2]
                # (cur_hist below is left uninitialised: every open node must be built or subtracted)
                assert nb + len(subtract) == nl, (d, nb, len(subtract), nl)
                if nb == nl and build == open_nodes:
                    cur_hist = mine
                else:
                    cur_hist = torch.empty((nl, shards.Bs, 2), dtype=torch.int64, device=dev)
                    if nb:
                        cur_hist.index_copy_(0, up[h_bidx], mine)
            if sub_t is not None:
                C.tree_hist_subtract(prev_hist, cur_hist, *sub_t, shards.Bs)
            with tracing.span("tree.split"):
                mine = _best_splits(C, cur_hist, totals, shards.boff, shards.nbins, shards.zbin, shards.fid_orig,
                                    node_ids, ws.kexp, params, feat_thr, tree_index, shards.Fa, shards.f0, **col_kw)
                with _CollTimer(dev):
                    allt = coll.all_gather(mine)                              # [S, nl, 5]
                gains = allt[:, :, 0].contiguous().view(torch.float64)
                best_s = torch.argmax(gains, dim=0)                           # ties -> lowest shard = lowest feature
                packed = allt[best_s, torch.arange(nl, device=dev)].cpu().numpy()
        # --- create children
        next_level, default_child, splits = tab.apply_splits(open_nodes, packed, d, Q, params, scale, max_nodes)
        if splits:
            with tracing.span("tree.partition"):
                _partition(C, Q, ws, default_child, splits)
        prev_hist = cur_hist
        prev_index = local
        level = next_level

    return tab.build(Q, params, scale)


def device_levels_ok(params: GrowParams, weight, device_levels: Optional[bool] = None) -> bool:
    """The device level loop covers every tree whose deepest level builds <= one pass of node
    slots: GBDT to depth 6, class-count trees to depth 7 (RF with per-node feature sampling,
    which builds every open node, to depth 7; weighted ones to depth 5)."""
    on = DEVICE_LEVELS if device_levels is None else device_levels
    deepest = 2 ** max(params.max_depth - (1 if params.feat_k else 2), 0)
    return on and deepest <= slots_per_tile(_choose_np(params, weight)) * MAX_CT


class LevelState:
    """Device buffers of the level loop (node table, ping-pong open lists, partition and plan
    tables), allocated once per workspace and depth."""

    def record_event(self, stream=None):
        """An event recorded on ``stream`` (default: the current stream; a reused event on the
        device, _Done on the host). Passing the stream saves a torch.cuda.current_stream() lookup
        (~10 us of host time per call)."""
        if self._events is None:
            return _Done()
        ev = self._events[self._ev_i]
        self._ev_i = (self._ev_i + 1) % len(self._events)
        ev.record(stream)
        return ev

    def host_views(self, buf: torch.Tensor) -> dict:
        """Named views of a host copy of the arena (node table fields + exponents)."""
        return {name: buf[o:o + n].view(dt).view(shape) for name, dt, shape, o, n in self._layout}

    def __init__(self, Q: Quantized, max_depth: int, n_sel: int = 0):
        dev = Q.device
        M = 2 ** (max_depth + 1)
        cap = 2 ** max_depth
        # RF levels with preselected item lists (PRESELECT): per level the 4 plan counts, then
        # 8 per-XCD active-item counts per sampled item group, read by the host in one copy
        self.n_sel = n_sel
        self.rf_thr = [torch.empty(cap, dtype=torch.float64, device=dev) for _ in range(2)] if n_sel else None
        self.rf_mask = [torch.empty(Q.Fa, dtype=torch.uint8, device=dev) for _ in range(2)] if n_sel else None
        i32 = lambda n: torch.full((n,), -1, dtype=torch.int32, device=dev)   # noqa: E731
        self.M, self.cap, self.max_depth = M, cap, max_depth
        # the node table (+ the tree's quantisation exponents) lives in ONE device arena, mirrored by
        # one pinned host arena: the host reads a finished tree with a single D2H copy (eleven
        # separate small copies cost ~0.4 ms per tree at ~25-30 us each)
        layout = [("stats", torch.int64, (M, 2)), ("gain", torch.float64, (M,)), ("n_nodes", torch.int32, (1,)),
                  ("kexp", torch.int32, (2,)), ("parent", torch.int32, (M,)), ("feat", torch.int32, (M,)),
                  ("bin", torch.int32, (M,)), ("left", torch.int32, (M,)), ("right", torch.int32, (M,)),
                  ("leaf", torch.uint8, (M,))]
        offs, nbytes = [], 0
        for _, dt, shape in layout:
            isz = torch.empty(0, dtype=dt).element_size()
            nbytes = (nbytes + 7) // 8 * 8
            offs.append(nbytes)
            nbytes += isz * int(np.prod(shape))
        nbytes = (nbytes + 7) // 8 * 8         # (copied in 8-byte words by the GBDT prologue)
        self.arena = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.arena_host = torch.zeros(nbytes, dtype=torch.uint8)
        if dev.type == "cuda":
            self.arena_host = self.arena_host.pin_memory()
        self._layout = []
        for (name, dt, shape), o in zip(layout, offs):
            n = torch.empty(0, dtype=dt).element_size() * int(np.prod(shape))
            setattr(self, name if name != "kexp" else "kexp_slot", self.arena[o:o + n].view(dt).view(shape))
            self._layout.append((name, dt, shape, o, n))
        self.host = self.host_views(self.arena_host)
        self.n_nodes.fill_(1)
        for t_ in (self.parent, self.left, self.right, self.feat, self.bin):
            t_.fill_(-1)
        self.gain.fill_(-1.0)
        # the root state of every tree (node 0 only, stats filled per tree): one H2D copy of this
        # image replaces ~9 fill launches at the start of each tree
        self.arena_init = self.arena.to("cpu", copy=True)       # (a copy also when dev is the CPU)
        if dev.type == "cuda":
            self.arena_init = self.arena_init.pin_memory()
        self.arena_init_dev = self.arena.clone()       # (the fused GBDT prologue copies it in on the device)
        self.zero1 = torch.zeros(1, dtype=torch.int32, device=dev)      # the root level's slot -> row table
        self.open = [i32(cap), i32(cap)]
        self.totals = [torch.zeros((cap, 2), dtype=torch.int64, device=dev) for _ in range(2)]
        self.counts = torch.zeros((max_depth + 1, 4 + 8 * n_sel), dtype=torch.int32, device=dev)
        self.counts_host = torch.zeros((max_depth + 1, 4 + 8 * n_sel), dtype=torch.int32)
        if dev.type == "cuda":
            self.counts_host = self.counts_host.pin_memory()
        self.one = torch.ones(1, dtype=torch.int32, device=dev)
        # events the level loop records for the host (re-recorded round robin: each one is waited on
        # before the loop records four more)
        self._events = [torch.cuda.Event() for _ in range(4)] if dev.type == "cuda" else None
        self._ev_i = 0
        self.default_child, self.node_slot = i32(M), i32(M)
        self.cs = [i32(cap) for _ in range(5)]          # feat, default, other, bin, left_default
        self.s2n, self.sub_dst, self.sub_par, self.sub_sib = i32(cap), i32(cap), i32(cap), i32(cap)
        self.sub_of = i32(cap)          # (runner levels) open index -> subtraction slot (-1)
        # data-parallel levels (tree.h LevelRowsArgs): histogram row per open node (level parity)
        # and the subtraction triples as rows
        self.row_of = [i32(cap), i32(cap)]
        self.dst_row, self.par_row, self.sib_row = i32(cap), i32(cap), i32(cap)
        # (the partition splits on dense-block features in its row pass, not the CSC column pass)
        self.node_dense = self.hot_row = None
        if Q.dense is not None:
            hot_row = np.full(Q.Fa, -1, dtype=np.int32)
            hot_row[Q.hot] = np.arange(len(Q.hot), dtype=np.int32)
            self.hot_row = torch.from_numpy(hot_row).to(dev)
            self.node_dense = i32(4 * M)


def grow_tree_device(Q: Quantized, ws: Workspace, params: GrowParams, tree_index: int, g: torch.Tensor,
                     h: torch.Tensor, weight: Optional[torch.Tensor] = None, coll=None,
                     shards: Optional["FeatureShards"] = None, label: Optional[torch.Tensor] = None,
                     bootstrap: bool = False, deferred: bool = False, on_first_wait=None,
                     margin: Optional[torch.Tensor] = None):
    """One tree through :func:`device_tree_steps`, waiting on each event it yields."""
    batcher = LevelBatcher(coll, shards.S, Q.device) if shards is not None else None
    return drive(device_tree_steps(Q, ws, params, tree_index, g, h, weight, coll, shards, label, bootstrap,
                                   deferred, on_first_wait, margin), batcher)


def _wide_features(nbins: torch.Tensor, Fa: int) -> torch.Tensor:
    """Indices of the features with > 16 bins (split_wide_kernel), memoised on the nbins tensor."""
    memo = getattr(nbins, "_fdx_wide", None)
    if memo is None or memo[0] != Fa:
        idx = np.nonzero(nbins[:Fa].cpu().numpy() > 16)[0].astype(np.int32)
        memo = (Fa, torch.from_numpy(idx).to(nbins.device))
        nbins._fdx_wide = memo
    return memo[1]


def _level_runner(Q: Quantized, ws: Workspace, st: "LevelState", params: GrowParams, item_groups: list,
                  sampled: bool):
    """The lane's native level runner (csrc/bindings_level.cpp RfLevels), built once per workspace,
    level state and tree parameters. RF (``sampled``): every kernel of a level; GBDT: the tree
    prologue, the fused split + plan and the partition (the row-group passes stay in Python)."""
    key = (params.mode, params.max_depth, params.min_gain, params.min_child, params.seed, params.feat_k,
           params.lambda_, sampled, params.subsample, params.colsample_bytree, params.colsample_bylevel,
           params.colsample_bynode)
    cached = getattr(ws, "_rf_runner", None)
    if cached is not None and cached[0] is st and cached[1] == key:
        return cached[2]
    cfg = dict(groups=[(g.item_start, g.item_end, g.item_f0, g.item_meta, g.wave_order(), int(g.bt))
                       for g in item_groups],
               h_row=Q.h_row if sampled else None, h_key=Q.h_key if sampled else None, csc_row=Q.csc_row,
               csc_bin=Q.csc_bin, colptr=Q.colptr, nbins=Q.nbins,
               zbin=Q.zbin, fid_orig=Q.fid_orig, dense=Q.dense if st.node_dense is not None else None,
               hot_row=st.hot_row, rowdig=ws.rowdig, rowpack=ws.rowpack() if sampled else None, row_node=ws.row_node,
               kexp=ws.kexp, build_all=bool(params.feat_k), arena_stats=st.stats[0], open0=st.open[0],
               totals0=st.totals[0], kexp_slot=st.kexp_slot,
               stats=st.stats, parent=st.parent, left=st.left, right=st.right, feat=st.feat, bin=st.bin, leaf=st.leaf,
               gain=st.gain, n_nodes=st.n_nodes, counts=st.counts, counts_host=st.counts_host,
               default_child=st.default_child, cs_feat=st.cs[0], cs_default=st.cs[1], cs_other=st.cs[2],
               cs_bin=st.cs[3], cs_left_default=st.cs[4], node_slot=st.node_slot, s2n=st.s2n, sub_dst=st.sub_dst,
               sub_par=st.sub_par, sub_sib=st.sub_sib, sub_of=st.sub_of, node_dense=st.node_dense, mode=int(params.mode),
               max_depth=int(params.max_depth), min_gain=float(params.min_gain), lambda_=float(params.lambda_),
               mcw=float(params.min_child), seed=int(params.seed), subsample=float(params.subsample),
               keepbits=ws.keepbits(params),
               F=int(Q.num_features), k=int(params.feat_k),
               lds=bool(RF_LDS), wps=int(PARTITION_WPS), arena=st.arena, dig16=ws.dig16() if sampled else None)
    col = ColumnSampler.of(Q, ws, params)
    if col is not None:
        cfg.update(col.runner_cfg())
    runner = native.lib().RfLevels(cfg)
    ws._rf_runner = (st, key, runner)
    return runner


# the DP runner calls RCCL directly on the process group's communicator (0: through Python)
DP_DIRECT_RCCL = os.environ.get("FDX_DP_DIRECT_RCCL", "1") == "1"


def _gbdt_setup(Q, ws, st, params, runner, rg, shards=None, coll=None) -> torch.Tensor:
    """Hands the runner the row-group tables and fixed level buffers of its C++ GBDT level loop
    (RfLevels.gbdt_setup), once per runner: one process, the two level-histogram tensors; data
    parallel (``shards``), the shard-major send buffer, the two reduced-level buffers, the feature
    shard's split tables and the collectives (RCCL communicator, Python callbacks). Returns what
    the prologue zeroes for the root level: row 0 of the first histogram tensor, or the root's
    send region."""
    key = (RG_DBG, GBDT_CHOOSE_ROWS, PARTITION_COUNTS, RG_PARTIALS, qmod.RG_LIST_WGS, qmod.RG_ALPHA,
           qmod.RG_EM_MIN_FRAC)
    cached = getattr(ws, "_gbdt_levels", None)
    if cached is not None and cached[0] is runner and cached[1] is shards and cached[2] == key:
        return cached[3]                                                    # (in-process A/Bs flip these)
    dev, D = Q.device, int(params.max_depth)
    em = rg.erow is not None and qmod.RG_EM_MIN_FRAC <= 1.0
    cfg = dict(
        rg_wg_list=rg.list_work(), rg_wg_first_list=rg.list_work_first() if RG_PARTIALS else None,
        rg_ptr=rg.ptr, rg_ent=rg.ent, rg_gbase=rg.gbase, rg_gbin=rg.gbin, rg_gmode=rg.gmode, rg_wg=rg.work(),
        rg_erow=rg.erow, rg_ebase=int(rg.ebase) if rg.erow is not None else 0,
        emdig=ws.rg_emdig() if em else None, em_min_rows=max(1, int(qmod.RG_EM_MIN_FRAC * Q.n_rows)),
        rg_part=ws.rg_part(rg, rg.list_work()) if RG_PARTIALS else None,
        rg_wg_first=rg.work_first() if RG_PARTIALS else None,
        list_work=ws.rg_work, rg_start=ws.rg_start, rg_list=ws.rg_list, rg_listdig=ws.rg_listdig,
        one=st.one, zero1=st.zero1, open1=st.open[1], totals1=st.totals[1], boff=Q.boff,
        counted=PARTITION_COUNTS, dbg=RG_DBG, choose_rows=GBDT_CHOOSE_ROWS)
    if shards is None:
        # level d opens at most 2^d nodes; even and odd levels alternate between the two tensors
        rows = [max([1] + [1 << d for d in range(k, D, 2)]) for k in (0, 1)]
        hists = [torch.empty((r, Q.TB, 2), dtype=torch.int64, device=dev) for r in rows]
        cfg.update(hist_a=hists[0], hist_b=hists[1], wide=_wide_features(Q.nbins, Q.Fa),
                   packed=torch.empty((1 << (D - 1), 5), dtype=torch.int64, device=dev))
        root = hists[0][:1]
    else:
        S, Bs = int(shards.S), int(shards.Bs)
        widest = max(1 << max(D - 1, 1), 2)
        send = torch.empty(S * widest * Bs * 2, dtype=torch.int64, device=dev)
        outs = [torch.empty((widest, Bs, 2), dtype=torch.int64, device=dev) for _ in range(2)]
        cb = _DpCollectives(coll, dev)
        comm, lib = _rccl_comm(dev)
        cfg.update(comm=comm, rccl_lib=lib, rs=cb.rs, ag=cb.ag, mx=cb.mx, S=S, Bs=Bs, bin_lo=shards.bin_lo, send=send,
                   out_a=outs[0], out_b=outs[1], row_of0=st.row_of[0], row_of1=st.row_of[1],
                   ag_in=torch.empty((widest, 5), dtype=torch.int64, device=dev), sboff=shards.boff,
                   snbins=shards.nbins, szbin=shards.zbin, sfid=shards.fid_orig, f0=int(shards.f0),
                   swide=_wide_features(shards.nbins, shards.Fa), dst_row=st.dst_row, par_row=st.par_row,
                   sib_row=st.sib_row, iota=ws.iota(64))
        root = send[:S * 2 * Bs * 2]
    runner.gbdt_setup(cfg)
    ws._gbdt_levels = (runner, shards, key, root)
    if shards is not None and runner.dp_direct() and runner not in _DP_RUNNERS:
        _DP_RUNNERS.append(runner)
    return root


class _Driver(enum.Enum):
    """Who runs a tree's prologue and its levels: exactly one per tree."""
    CXX_GBDT = "cxx"        # the runner's C++ GBDT loop (_cxx_gbdt_tree): no level of the generic loop
    RUNNER = "runner"       # the generic loop behind the runner's fused prologue (one process)
    PYTHON = "python"       # the generic loop behind the prologue issued launch by launch (host twins,
    #                         data parallel, trees without a runner)


class _Path(NamedTuple):
    """How one tree runs, resolved once (_resolve_tree); every stage below reads it."""
    np_: int                # digit planes per statistic (_choose_np)
    build_all: bool         # per-node feature sampling: every open node built, no sibling subtraction
    sampled: bool           # ... of class counts (np_ = 1): the packed sampled passes
    presel: bool            # levels >= 1 launch from item lists compacted with the previous plan
    sel_ids: tuple          # ... the item groups that have items
    item_groups: list       # the CSC item groups of the sampled passes
    runner: object          # the native level runner (RfLevels) or None
    dp: bool                # feature shards: a level splits around a reduce-scatter and an all-gather
    compact: bool           # ... which carry only the bins of the level's sampled features
    col: Optional[ColumnSampler]
    driver: _Driver


# what the stages of one tree work on (stream: the one current when the tree started; the forest
# driver advances a lane inside that lane's stream context)
_TreeCtx = namedtuple("_TreeCtx", "C Q ws st params tree seed shards coll stream")
# a tree's row statistics as given: GBDT g, h (or margin and label to compute them from), class
# counts label / weight / bootstrap
_TreeInput = namedtuple("_TreeInput", "g h label weight bootstrap margin")
# a level's feature sample: RF thresholds per open node + union mask (GBDT column sampling: the
# node stage's thresholds, tree_split_find's arguments in col_kw); compact levels: the sampled
# features' bin offsets; data parallel: the bins per shard row
_Sample = namedtuple("_Sample", "thr mask col_kw local Bs")
# where a level's histogram passes add: tensor, bin offset per feature, row stride, slot -> row
_HistOut = namedtuple("_HistOut", "target boff stride s2n")
# what the CSC passes read per row: slot bytes (None: every row in slot 0), digit words, the
# sampled passes' packed word (None: the root kernel on ``dig``)
_RowState = namedtuple("_RowState", "slot8 dig pack")


# one level of the generic loop as the host sizes it (the previous plan's counts). cur: parity of
# the ping-pong level buffers; per_xcd: sampled item group -> its largest per-XCD active-item count
# (PRESELECT, d > 0); more: a level follows; open / totals: the open nodes' ids and exact sums
_Level = namedtuple("_Level", "d cur n_open n_build per_xcd more open totals n_open_ptr")


def _resolve_tree(Q, ws, params, tree_index, inp: _TreeInput, coll, shards) -> tuple:
    """(_TreeCtx, _Path) of one tree: level state, runner and driver."""
    dev = Q.device
    cuda = dev.type == "cuda"
    np_ = _choose_np(params, inp.weight)
    build_all = bool(params.feat_k)
    sampled = build_all and np_ == 1
    # RF levels >= 1: the next level's feature sample and its active-item lists are queued right
    # after the plan, so the per-XCD item counts reach the host with the level's counts and each
    # histogram pass launches one wave per active item (no grid of ~300K mostly idle wave slots)
    presel = PRESELECT and sampled and cuda
    item_groups = (Q.groups + Q.hot_groups) if sampled else []
    sel_ids = tuple(gi for gi, grp in enumerate(item_groups) if grp.num_items) if presel else ()
    st = getattr(ws, "_levels", None)
    if st is None or st.max_depth != params.max_depth or st.n_sel != len(sel_ids):
        st = ws._levels = LevelState(Q, params.max_depth, len(sel_ids))
    # the native runner: RF levels and GBDT levels (any world size). A single process also fuses
    # the GBDT prologue and the split + plan; under data parallelism the quantisation max is an
    # all-reduce and the levels split around the reduce-scatter / all-gather
    gbdt_native = NATIVE_LEVELS and cuda and params.mode == 0 and inp.weight is None and not build_all
    # (the runner's level 0 completes the root's sums: at least one level)
    runner = _level_runner(Q, ws, st, params, item_groups, sampled) \
        if (NATIVE_LEVELS and cuda and (sampled or gbdt_native) and params.max_depth >= 1) else None
    dp = shards is not None
    fused_prologue = runner is not None and not dp and coll is None
    # GBDT rounds on the row-group engine, in one process or data parallel: the level loop runs in
    # the runner (RfLevels.gbdt_levels; data parallel: around the level's collectives, RCCL called
    # by the runner or Python callbacks)
    if (runner is not None and (dp or fused_prologue) and gbdt_native and GBDT_CXX_LEVELS and np_ == 4 and
            inp.margin is not None and inp.g is None and ws.rowgroups() is not None):
        driver = _Driver.CXX_GBDT
    else:
        driver = _Driver.RUNNER if fused_prologue else _Driver.PYTHON
    # RF under data parallelism: each level reduce-scatters only its sampled features' bins; level
    # d + 1's sample and layout are computed right after level d's plan, so their shard sizes reach
    # the host with the level's counts (one wait per level; the root's before the loop)
    compact = dp and build_all and 0 < params.feat_k < Q.num_features and \
        (RF_COMPACT == "1" or (RF_COMPACT == "auto" and shards.S > 1))
    cx = _TreeCtx(native.lib(), Q, ws, st, params, int(tree_index), int(params.seed), shards, coll,
                  torch.cuda.current_stream(dev) if cuda else None)
    return cx, _Path(np_, build_all, sampled, presel, sel_ids, item_groups, runner, dp, compact,
                     ColumnSampler.of(Q, ws, params), driver)


def _quantise(C, Q, ws, params, tree_index, inp: _TreeInput, np_: int, coll, max_only: bool = False) -> None:
    """The tree's quantisation launch by launch: max |statistic| into ws.maxabs (all-reduced under
    ``coll``) -> digits, exponents and totals (``max_only``: left to the runner's prologue); class
    counts in one plane need no max."""
    seed, mode_rs, mx = int(params.seed), 0 if params.mode == 0 else 1, None
    if np_ == 4:
        C.tree_quant_max(inp.g, inp.h, inp.label, inp.weight, seed, int(tree_index), bool(inp.bootstrap), mode_rs,
                         Q.n_rows, ws.maxabs, Q.row0)
        mx = coll.max(ws.maxabs) if coll is not None else ws.maxabs
    if not max_only:
        C.tree_quant(inp.g, inp.h, inp.label, inp.weight, seed, int(tree_index), bool(inp.bootstrap), mode_rs, np_, mx,
                     ws.rowdig, ws.kexp, ws.totals, ws.digp, Q.row0,
                     *((float(params.subsample), ws.keepbits(params)) if np_ == 4 else ()))


def _runner_prologue(cx: _TreeCtx, p: _Path, inp: _TreeInput) -> torch.Tensor:
    """Driver RUNNER: gradients, max, arena image, zeroed root histogram and quantisation in the
    runner's prologue (2 launches for a GBDT round); the root's sums stay in the quantisation's
    slots, completed by the runner's level 0. Returns the root histogram."""
    Q, ws, st, runner = cx.Q, cx.ws, cx.st, p.runner
    pre_hist = torch.empty((1, Q.TB, 2), dtype=torch.int64, device=Q.device)     # zeroed by the prologue
    with tracing.span("tree.quant"):
        # (the dense-block digit planes only feed the MFMA dense path, off with the row groups)
        digp = ws.digp if (ws.digp is not None and not p.build_all and ws.rowgroups() is None) else None
        if p.np_ == 4 and inp.margin is not None and inp.g is None:
            g, h = ws.gh()
            runner.prologue(inp.margin, g, h, inp.label, None, cx.tree, False, 4, None, ws.totals, digp, Q.row0,
                            pre_hist, st.arena_init_dev)
        else:
            # arena image first: the quantisation adds the root totals into it
            st.arena.copy_(st.arena_init, non_blocking=True)
            _quantise(cx.C, Q, ws, cx.params, cx.tree, inp, p.np_, None, max_only=True)
            runner.prologue(None, inp.g, inp.h, inp.label, inp.weight, cx.tree, bool(inp.bootstrap), p.np_,
                            ws.maxabs if p.np_ == 4 else None, ws.totals, digp, Q.row0, pre_hist, None)
    if p.col is not None:
        runner.col_begin(cx.tree)
    return pre_hist


def _python_prologue(cx: _TreeCtx, p: _Path, inp: _TreeInput) -> None:
    """Driver PYTHON: gradients, quantisation, arena image and root (node 0, open list [0] with the
    exact totals, no host round trip; under data parallelism the totals are summed by the root
    level's reduce-scatter, LaneBufs.tot_bin), one launch each."""
    C, ws, st, coll = cx.C, cx.ws, cx.st, cx.coll
    if inp.margin is not None and inp.g is None:
        g, h = ws.gh()
        C.tree_logistic_grad(inp.margin, inp.label, inp.weight, g, h)
        inp = inp._replace(g=g, h=h)
    ws.row_node.zero_()
    with tracing.span("tree.quant"):
        _quantise(C, cx.Q, ws, cx.params, cx.tree, inp, p.np_, coll)
    st.arena.copy_(st.arena_init, non_blocking=True)
    st.open[0][:1].zero_()
    if not p.dp:
        tot = coll.sum(ws.totals) if coll is not None else ws.totals
        st.stats[0].copy_(tot)
        st.totals[0][:1].copy_(tot[None])
    # GBDT column sampling: the tree's and every level's stage thresholds, queued behind the prologue
    if p.col is not None and p.runner is not None:
        p.runner.col_begin(cx.tree)
    elif p.col is not None:
        p.col.begin(C, cx.seed, cx.tree)


def _cxx_gbdt_tree(cx: _TreeCtx, p: _Path, inp: _TreeInput, on_first_wait) -> None:
    """Driver CXX_GBDT, the whole tree: the prologue (gradients + max |g|, |h|, all-reduced by the
    runner under data parallelism + arena image + the root histogram or the root's send region
    zeroed, then the quantisation), level 0 queued, the previous tree's host table built while it
    runs (``on_first_wait``), then levels 1.. with the host waits inside the runner: the launches
    and trees of the generic loop."""
    Q, ws, st, runner = cx.Q, cx.ws, cx.st, p.runner
    with tracing.span("tree.quant"):
        root_zero = _gbdt_setup(Q, ws, st, cx.params, runner, ws.rowgroups(), cx.shards, cx.coll)
        g, h = ws.gh()
        runner.prologue(inp.margin, g, h, inp.label, None, cx.tree, False, 4, None, ws.totals, None, Q.row0,
                        root_zero, st.arena_init_dev)
    if p.col is not None:
        runner.col_begin(cx.tree)
    runner.gbdt_root(cx.tree)
    if on_first_wait is not None:
        on_first_wait()
    shape = runner.gbdt_levels(cx.tree)
    for j in range(0, len(shape), 2):
        LEVEL_STATS["levels"] += 1
        LEVEL_STATS["built_nodes"] += shape[j + 1]
        LEVEL_STATS["hist_bytes"] += shape[j + 1] * Q.TB * 16


def _open_level(cx: _TreeCtx, p: _Path, d: int) -> Optional[_Level]:
    """Level ``d`` as the host sizes it: the root, or the previous plan's counts (waited for by the
    caller); None when no node is open. Counts the level in LEVEL_STATS."""
    st, cur = cx.st, d % 2
    n_open = n_build = 1
    per_xcd = {}
    if d > 0:
        cnt = st.counts_host[d - 1].tolist()
        n_open, n_build = int(cnt[1]), int(cnt[2])
        if n_open == 0:
            return None
        for j, gi in enumerate(p.sel_ids):      # largest per-XCD active-item count of each sampled group
            active = cnt[4 + 8 * j: 12 + 8 * j]
            per_xcd[gi] = max(active)
            if per_xcd[gi]:           # (launch_hist: (npx + 3) / 4 x 8 workgroups of 4 waves)
                LEVEL_STATS["listed_passes"] += 1
                LEVEL_STATS["listed_active_items"] += sum(active)
                LEVEL_STATS["listed_grid_waves"] += (per_xcd[gi] + 3) // 4 * 8 * 4
    LEVEL_STATS["levels"] += 1
    LEVEL_STATS["built_nodes"] += n_build
    LEVEL_STATS["hist_bytes"] += n_build * cx.Q.TB * 16          # (g, h) int64 partials of the built nodes
    totals = st.totals[cur][:n_open]
    if d == 0 and p.driver is _Driver.RUNNER:
        totals = st.stats[:1]             # (unread: the runner sums the prologue's root slots)
    return _Level(d, cur, n_open, n_build, per_xcd, d + 1 < cx.params.max_depth, st.open[cur][:n_open], totals,
                  st.one if d == 0 else st.counts[d - 1, 1:2])


def _level_sample(cx: _TreeCtx, p: _Path, lv: _Level) -> _Sample:
    """RF: the exact k-of-F feature sample per open node and the level's union mask (compact and
    preselected levels: queued with the previous plan). GBDT column sampling: the node stage."""
    C, Q, st = cx.C, cx.Q, cx.st
    thr = mask = local = None
    Bs = cx.shards.Bs if p.dp else None
    if p.compact:
        thr, mask, local, Bs = cx.shards.compact_level(lv.cur, lv.n_open)
    elif p.sel_ids and lv.d > 0:
        thr, mask = st.rf_thr[lv.cur][:lv.n_open], st.rf_mask[lv.cur]
    elif p.build_all:
        thr = torch.empty(lv.n_open, dtype=torch.float64, device=Q.device)
        mask = torch.empty(Q.Fa, dtype=torch.uint8, device=Q.device)
        C.tree_rf_sample(cx.seed, cx.tree, lv.open, int(Q.num_features), int(cx.params.feat_k), Q.fid_orig, thr, mask,
                         None)
    col_kw = {}
    if p.col is not None and p.runner is not None:
        p.runner.col_level(lv.d, lv.open, cx.tree)       # (node stage queued; find() reads the tables)
    elif p.col is not None:
        thr, col_kw = p.col.level_args(C, cx.seed, cx.tree, lv.d, lv.open)
    return _Sample(thr, mask, col_kw, local, Bs)


def _hist_out(cx: _TreeCtx, p: _Path, lv: _Level, smp: _Sample, bufs, pre_hist) -> _HistOut:
    """One process: the level's [n_open, TB, 2] histograms (``pre_hist`` when the previous level
    queued their zero fill). Data parallel: this tree's rows of the batch's shard-major send buffer
    (``bufs``, a LaneBufs), slot k -> partial row k; compact levels send only the sampled bins."""
    Q, st = cx.Q, cx.st
    if p.dp:
        target = bufs.prepare(cx.ws.totals if lv.d == 0 else None)
        if p.runner is not None:      # (the runner's kernels add the shard offsets themselves)
            boff = smp.local if p.compact else cx.shards._local
        else:
            boff = cx.shards.boff_batched(bufs.shard_bins, smp.local)
        return _HistOut(target, boff, bufs.Bs, cx.ws.iota(lv.n_build))
    if pre_hist is not None and pre_hist.shape[0] >= lv.n_open:
        hist = pre_hist[:lv.n_open]
    else:
        hist = torch.zeros((lv.n_open, Q.TB, 2), dtype=torch.int64, device=Q.device)
    return _HistOut(hist, Q.boff, Q.TB, st.s2n[:lv.n_build] if lv.d > 0 else st.zero1)


def _row_pass(cx: _TreeCtx, p: _Path, lv: _Level, rg) -> _RowState:
    """The row pass in front of a level's CSC passes (none at the root, on the row-group engine,
    which lists the built rows from row_node itself, and on sampled levels with FUSED_PACK, which
    read the packed row state the previous level's partition wrote). A single built node: the
    passes run the root kernel on digit words zeroed outside it (no per-entry slot gather, no
    compaction; zero rows add nothing)."""
    C, ws, st = cx.C, cx.ws, cx.st
    if lv.d == 0:
        return _RowState(None, ws.rowdig, None)
    fused = p.sampled and FUSED_PACK
    single = lv.n_build == 1 and rg is None and not fused
    if single and getattr(ws, "rowdig_masked", None) is None:
        ws.rowdig_masked = torch.empty_like(ws.rowdig)
    if rg is None and not fused:
        if p.sampled and not single:
            C.tree_slot_pack(ws.row_node, st.node_slot, lv.n_build, ws.rowdig, ws.rowpack())
        else:
            C.tree_slot8(ws.row_node, st.node_slot, 0, lv.n_build, ws.slot8, ws.rowdig if single else None,
                         ws.rowdig_masked if single else None)
    pack = ws.rowpack() if (p.sampled and not single) else None
    return _RowState(None, ws.rowdig_masked, pack) if single else _RowState(ws.slot8, ws.rowdig, pack)


def _rowgroup_pass(cx: _TreeCtx, p: _Path, lv: _Level, rg, out: _HistOut, bufs, counted: bool) -> None:
    """GBDT: the level's histograms from the row-group CSR (root: every row; below: the row lists
    of the built nodes). ``counted``: the previous partition wrote the lists' counts."""
    C, Q, ws, st = cx.C, cx.Q, cx.ws, cx.st
    shard_args = (cx.shards.bin_lo, bufs.shard_bins) if p.dp else (None, 0)
    root = lv.d == 0
    # per-workgroup partial tables summed by one reduction instead of every workgroup's atomics on
    # the same bins (RgHistArgs part); the listed levels have their own, smaller work table
    wtab = rg.work() if root else rg.list_work()
    part = dict(part=ws.rg_part(rg, rg.list_work()), wg_first=rg.work_first() if root else rg.list_work_first()) \
        if (RG_PARTIALS and Q.device.type == "cuda") else {}
    if root:
        C.tree_rg_hist(rg.ptr, rg.ent, rg.gbase, rg.gbin, ws.rowdig, p.np_, None, None, None, 1, rg.gmode, wtab, out.s2n,
                       out.target, out.stride, *shard_args, RG_DBG, **rg.em_args(), **part)
        return
    # one built node: every row's digit words zeroed outside it, for the entry-major pass of the
    # sparse groups (taken when the node is large)
    emdig = ws.rg_emdig() if (lv.n_build == 1 and rg.erow is not None and qmod.RG_EM_MIN_FRAC <= 1.0) else None
    C.tree_rg_list(ws.row_node, st.node_slot, None, Q.n_rows, lv.n_build, ws.rg_work, ws.rg_start, ws.rg_list,
                   ws.rowdig, ws.rg_listdig, emdig, counted=counted, keepbits=ws.keepbits(cx.params))
    C.tree_rg_hist(rg.ptr, rg.ent, rg.gbase, rg.gbin, ws.rowdig, p.np_, ws.rg_list, ws.rg_start, ws.rg_listdig,
                   lv.n_build, rg.gmode, wtab, out.s2n, out.target, out.stride, *shard_args, RG_DBG,
                   **(rg.em_args(emdig) if emdig is not None else {}), **part)


def _sampled_lists(cx: _TreeCtx, p: _Path, lv: _Level) -> list:
    """Per item group of a sampled pass its (item list, count, per-XCD launch size): preselected
    (exactly one wave per active item, the list built with the previous level's plan); compacted
    by the pass itself while few items are active (<= LISTED_MAX_NODES open nodes: ~0.16 vs
    0.19 ms at the root; with more, its fixed grid balances worse than a wave per slot,
    profiles/r3s3/rf_probe_chunks.txt); or (None, None, -1): a wave per item slot."""
    out = []
    for gi, grp in enumerate(p.item_groups):
        if grp.num_items and p.sel_ids and lv.d > 0:
            j = p.sel_ids.index(gi)
            out.append((cx.ws.item_list(gi, grp)[0], cx.st.counts[lv.d - 1, 4 + 8 * j: 12 + 8 * j], lv.per_xcd[gi]))
        elif grp.num_items and lv.n_open <= LISTED_MAX_NODES:
            out.append((*cx.ws.item_list(gi, grp), -1))
        else:
            out.append((None, None, -1))
    return out


def _sampled_pass(cx: _TreeCtx, p: _Path, lv: _Level, feat_mask, rows: _RowState, out: _HistOut, bufs) -> None:
    """RF: the class-count histograms of the sampled features' CSC items, one runner call or one
    launch per item group on the side streams."""
    C, Q = cx.C, cx.Q
    lists = _sampled_lists(cx, p, lv)
    if p.runner is not None:
        p.runner.hist(lv.n_build, out.target, out.boff, feat_mask, out.s2n, rows.pack, [t[0] for t in lists],
                      [t[1] for t in lists], [t[2] for t in lists], cx.shards._shard_of if p.dp else None,
                      bufs.shard_bins if p.dp else 0)
        return
    ct = pass_ct(p.np_, lv.n_build)
    cx.ws.run_concurrent([functools.partial(
        C.tree_hist_sampled, grp.item_start, grp.item_end, grp.item_f0, grp.item_meta, grp.wave_order(), Q.h_row,
        Q.h_key, rows.pack, rows.dig, out.boff, Q.nbins, out.s2n, out.target, out.stride, grp.bt, ct, feat_mask, lst,
        cnt, RF_LDS, npx) for grp, (lst, cnt, npx) in zip(p.item_groups, lists) if grp.num_items])


def _csc_dense_launches(C, Q, ws, np_: int, n_slots: int, root: bool, use_dense: bool, rows: _RowState, feat_mask,
                        out: _HistOut) -> list:
    """The launches of one CSC histogram pass over ``n_slots`` node slots: every item group's
    (``use_dense``: the cold features' only, the hot features streamed from the dense block)."""
    ct = pass_ct(np_, n_slots)
    launches = []
    for grp in (Q.groups if use_dense else Q.groups + Q.hot_groups):
        if grp.num_items:
            launches.append(functools.partial(
                C.tree_hist_build, grp.item_start, grp.item_end, grp.item_f0, grp.item_meta, grp.wave_order(),
                Q.h_row, Q.h_key, rows.slot8, rows.dig, out.boff, Q.nbins, out.s2n, out.target, out.stride, grp.bt, ct,
                np_, feat_mask))
    if use_dense:
        for bt in (1, 2, 4):
            fg = C.tree_dense_fg(bt, 1 if root else ct)
            gfid, gden = ws.dense_groups(bt, fg)
            if gfid.numel():
                launches.append(functools.partial(
                    C.tree_hist_dense, Q.dense, ws.digp, ws.rowdig, None if root else ws.slot8_pad, gfid, gden,
                    out.boff, Q.nbins, out.s2n, out.target, out.stride, Q.n_rows, DENSE_RANGE_ROWS, bt, ct, np_))
    return launches


def _level_hist(cx: _TreeCtx, p: _Path, lv: _Level, smp: _Sample, out: _HistOut, bufs, rg, counted: bool) -> None:
    """The histograms of the level's built nodes into ``out``: the row-group engine (``rg``), the
    sampled RF passes, or the CSC items plus, down to DENSE_MAX_DEPTH, the dense block."""
    rows = _row_pass(cx, p, lv, rg)
    if rg is not None:
        _rowgroup_pass(cx, p, lv, rg, out, bufs, counted)
    elif p.sampled:
        _sampled_pass(cx, p, lv, smp.mask, rows, out, bufs)
    else:
        # (RF levels read only the sampled features' CSC items)
        use_dense = cx.Q.dense is not None and lv.d <= DENSE_MAX_DEPTH and not p.build_all
        cx.ws.run_concurrent(_csc_dense_launches(cx.C, cx.Q, cx.ws, p.np_, lv.n_build, lv.d == 0, use_dense, rows,
                                                 smp.mask, out))


def _level_rows(cx: _TreeCtx, p: _Path, lv: _Level, out: _HistOut, bufs, prev: tuple) -> tuple:
    """(the level's histograms, the row of each open node or None = its index), the larger siblings
    subtracted from ``prev`` (the previous level's pair) unless the runner does it in its split
    search (one process: split_plan). Data parallel, after the reduce-scatter: rows at stride Bs,
    read in place by the split search; the root also takes its reduced totals."""
    C, st, nb = cx.C, cx.st, lv.n_build
    subtract = lv.d > 0 and not p.build_all
    if not p.dp:
        if subtract and p.runner is None:
            C.tree_hist_subtract(prev[0], out.target, st.sub_dst[:nb], st.sub_par[:nb], st.sub_sib[:nb], cx.Q.TB)
        return out.target, None
    if lv.d == 0:
        tot = bufs.reduced_totals()
        st.stats[0].copy_(tot)
        lv.totals.copy_(tot[None])
    if not subtract:
        # every open node built, slot k = open node k (tree.h level_plan): the reduced rows ARE
        # the level's histograms
        return bufs.mine(), None
    # the built rows stay where the collective wrote them and the subtraction fills rows after
    # them: per open node its row (tree.h LevelRowsArgs), no copy
    C.tree_level_rows(st.s2n, st.sub_dst, st.sub_par, prev[1], nb, bufs.row0, bufs.sub_base, st.row_of[lv.cur],
                      st.dst_row, st.par_row, st.sib_row)
    if LEVEL_CHECKS:
        n_sub = int((st.sub_dst[:nb] >= 0).sum())
        assert nb + n_sub == lv.n_open, (lv.d, nb, n_sub, lv.n_open)
    C.tree_hist_subtract(prev[0], bufs.out, st.dst_row[:nb], st.par_row[:nb], st.sib_row[:nb], bufs.Bs)
    return bufs.out, st.row_of[lv.cur][:lv.n_open]


def _split_search(cx: _TreeCtx, p: _Path, lv: _Level, smp: _Sample, hist, bufs, row_of):
    """The best split per open node over this rank's features. One process: the [n_open, 5]
    tuples (with a runner only their buffer: split_plan searches, reduces and plans in 2
    launches). Data parallel: this shard's tuples into ``bufs.ag_in`` for the all-gather (None)."""
    C, Q, ws, sh = cx.C, cx.Q, cx.ws, cx.shards
    if not p.dp:
        if p.runner is None:
            return _best_splits(C, hist, lv.totals, Q.boff, Q.nbins, Q.zbin, Q.fid_orig, lv.open, ws.kexp, cx.params,
                                smp.thr, cx.tree, Q.Fa, 0, cache=ws.split_cache, **smp.col_kw)
        packed = ws.split_cache.get(("out", lv.n_open))
        if packed is None:
            packed = ws.split_cache[("out", lv.n_open)] = torch.empty((lv.n_open, 5), dtype=torch.int64,
                                                                      device=Q.device)
        return packed
    boff = smp.local[sh.f0: sh.f0 + sh.Fa + 1] if p.compact else sh.boff
    if p.runner is not None:
        p.runner.split(hist, lv.totals, boff, sh.nbins, sh.zbin, sh.fid_orig, lv.open, smp.thr, cx.tree, sh.f0,
                       bufs.ag_in, row_of, _wide_features(sh.nbins, sh.Fa), lv.d if p.col is not None else -1)
    else:
        _best_splits(C, hist, lv.totals, boff, sh.nbins, sh.zbin, sh.fid_orig, lv.open, ws.kexp, cx.params, smp.thr,
                     cx.tree, sh.Fa, sh.f0, cache=ws.split_cache, out=bufs.ag_in, row_of=row_of, **smp.col_kw)
    return None


def _runner_plan_partition(cx: _TreeCtx, p: _Path, lv: _Level, smp: _Sample, hist, packed, prev_hist, rg) -> tuple:
    """Runner levels: (split search and) plan, the event the host waits on for the next level's
    counts, the partition. Returns (event, the next level's histograms zeroed by the partition or
    None, whether its row pass wrote the next level's row-list counts)."""
    Q, ws, st, sh, runner = cx.Q, cx.ws, cx.st, cx.shards, p.runner
    d, n_open, nxt = lv.d, lv.n_open, 1 - lv.cur
    sample_next = lv.more and (p.compact or bool(p.sel_ids))
    thr_n = mask_n = None
    lay = (None,) * 5 + (0,)
    if sample_next and p.compact:
        thr_n, mask_n = sh.compact_thr(nxt, 2 * n_open), sh.compact_mask(nxt)
        lay = (sh._fs_dev, Q.nbins, sh._local_c[nxt], sh._sizes[nxt], sh.sizes_host[nxt], sh.max_shard_features)
    elif sample_next:
        thr_n, mask_n = st.rf_thr[nxt], st.rf_mask[nxt]
    sel = [ws.item_list(gi, grp)[0] if gi in p.sel_ids else None for gi, grp in enumerate(p.item_groups)] \
        if (p.sel_ids and lv.more) else []
    if p.dp:
        runner.plan(d, n_open, packed, lv.open, lv.n_open_ptr, st.open[nxt], st.totals[nxt], cx.tree, sample_next,
                    thr_n, mask_n, *lay, sel)
    else:
        fused_sub = d > 0 and not p.build_all
        runner.split_plan(d, n_open, hist, lv.totals, Q.boff, smp.thr, cx.tree, packed, _wide_features(Q.nbins, Q.Fa),
                          lv.open, lv.n_open_ptr, st.open[nxt], st.totals[nxt], sample_next, thr_n, mask_n, sel,
                          prev_hist if fused_sub else None)
    ev = st.record_event(cx.stream)
    zero = None
    if not p.dp and lv.more and not p.build_all:
        zero = torch.empty((2 * n_open, Q.TB, 2), dtype=torch.int64, device=Q.device)
    counted = bool(lv.more and rg is not None and PARTITION_COUNTS and cx.C.tree_partition_counts_ok(Q.n_rows))
    with tracing.span("tree.partition"):
        runner.partition(d, n_open, bool(p.sampled and FUSED_PACK and lv.more), zero,
                         p.driver is _Driver.RUNNER and p.sampled, ws.rg_work if counted else None)
    return ev, zero, counted


def _python_plan_partition(cx: _TreeCtx, p: _Path, lv: _Level, packed) -> tuple:
    """Python levels: ``tree_level_plan``, the next level's sample and active-item lists, the
    counts' copy to the host and its event, the partition (sampled RF levels: the next level's
    packed row state written on the way). Returns (event, the next level's zeroed histograms or
    None)."""
    C, Q, ws, st, params = cx.C, cx.Q, cx.ws, cx.st, cx.params
    d, n_open, nxt = lv.d, lv.n_open, 1 - lv.cur
    C.tree_level_plan(packed, n_open, d, params.max_depth, int(params.mode), p.build_all, ws.kexp,
                      float(params.min_gain), Q.zbin, st.hot_row,
                      st.n_nodes, st.stats, st.parent, st.left, st.right, st.feat, st.bin, st.leaf, st.gain,
                      lv.open, lv.n_open_ptr, st.default_child, st.node_dense, *st.cs, st.counts[d],
                      st.open[nxt], st.totals[nxt], st.node_slot, st.s2n, st.sub_dst, st.sub_par, st.sub_sib)
    nxt_open = st.open[nxt][:2 * n_open]      # at most 2 n_open long, -1 padded (tree.h level_plan_reset)
    if p.compact and lv.more:
        cx.shards.sample_compact(C, nxt, cx.seed, cx.tree, nxt_open, int(Q.num_features), int(params.feat_k),
                                 Q.fid_orig)
    if p.sel_ids and lv.more:
        if p.compact:
            mask_n = cx.shards.compact_mask(nxt)
        else:
            mask_n = st.rf_mask[nxt]
            C.tree_rf_sample(cx.seed, cx.tree, nxt_open, int(Q.num_features), int(params.feat_k), Q.fid_orig,
                             st.rf_thr[nxt][:2 * n_open], mask_n, None)
        groups = [p.item_groups[gi] for gi in p.sel_ids]
        C.tree_hist_select_groups([[g.item_start, g.item_f0, g.item_meta, g.wave_order()] for g in groups], Q.nbins,
                                  mask_n, [ws.item_list(gi, g)[0] for gi, g in zip(p.sel_ids, groups)],
                                  st.counts[d, 4:].view(len(p.sel_ids), 8))
    st.counts_host[d].copy_(st.counts[d], non_blocking=Q.device.type == "cuda")
    ev = st.record_event(cx.stream)
    with tracing.span("tree.partition"):
        fuse = p.sampled and FUSED_PACK and lv.more
        C.tree_partition_cols(ws.row_node, st.default_child, *st.cs, st.counts[d], Q.colptr, Q.csc_row, Q.csc_bin,
                              st.node_dense, Q.dense if st.node_dense is not None else None, n_open, PARTITION_WPS,
                              *((st.node_slot, ws.rowdig, ws.rowpack()) if fuse else (None, None, None)))
    if p.dp or not lv.more:
        return ev, None
    return ev, torch.zeros((2 * n_open, Q.TB, 2), dtype=torch.int64, device=Q.device)


def _read_tree(cx: _TreeCtx, p: _Path, deferred: bool):
    """The end of every tree (a generator): one read of the node table, the arena (table +
    exponents) in one D2H copy and one wait; ``deferred`` GBDT trees return a PendingTree whose
    margin update reads the device node table (one launch with the runner)."""
    st, ws, params = cx.st, cx.ws, cx.params
    if p.driver is _Driver.PYTHON:         # (the runner's prologues write the exponents themselves)
        st.kexp_slot.copy_(ws.kexp)
    node_value = None
    if deferred and params.mode == 0:
        node_value = (p.runner, params) if p.runner is not None else leaf_values_device(st.stats, ws.kexp, params)
    st.arena_host.copy_(st.arena, non_blocking=True)
    cuda = cx.Q.device.type == "cuda"
    done = torch.cuda.Event() if cuda else _Done()
    if cuda:
        done.record(cx.stream)

    def finish() -> Tree:
        done.synchronize()
        return tree_from_host(cx.Q, params, st.host)

    if node_value is not None:
        return PendingTree(node_value, finish)
    yield done
    return finish()


def device_tree_steps(Q: Quantized, ws: Workspace, params: GrowParams, tree_index: int, g: torch.Tensor,
                      h: torch.Tensor, weight: Optional[torch.Tensor] = None, coll=None,
                      shards: Optional["FeatureShards"] = None, label: Optional[torch.Tensor] = None,
                      bootstrap: bool = False, deferred: bool = False, on_first_wait=None,
                      margin: Optional[torch.Tensor] = None):
    """A generator: yields an event wherever the host must wait for the device (the next level's
    counts, the finished node table) and returns the Tree (or PendingTree). :func:`drive` runs
    one tree; the forest driver (models/forest_batch.py) interleaves several on their own streams.

    One tree with the level loop on the device (same trees as grow_tree's host loop, bit for
    bit), by the driver _resolve_tree picks. The generic loop, per level: feature sample ->
    histogram passes -> sibling subtraction -> split search -> plan (the splits applied to the
    device node table, this level's partition tables, the next level's open list / builds /
    subtraction triples) -> partition. The host waits only for the plan's 16-byte counts (copied
    while the partition runs) to size the next level's launches, and reads the node table once at
    the end. Data parallel (``shards``): the built nodes' partial histograms are reduce-scattered
    by feature shard and the per-shard best splits all-gathered (the CollStep yields), stream-
    ordered on the device; every rank plans the identical next level from the gathered splits.
    ``deferred`` (GBDT): return a :class:`PendingTree` whose leaf values were computed on the
    device; the host table is built later (``on_first_wait`` of the next tree runs it while that
    tree's root level is on the GPU), so the GPU never idles on the host's tree build.
    ``margin`` (GBDT, with ``label`` and g = h = None): the round's gradients are computed here,
    fused into the tree's prologue when the native runner drives the levels."""
    inp = _TreeInput(g, h, label, weight, bootstrap, margin)
    cx, p = _resolve_tree(Q, ws, params, tree_index, inp, coll, shards)
    if p.driver is _Driver.CXX_GBDT:
        _cxx_gbdt_tree(cx, p, inp, on_first_wait)
        return (yield from _read_tree(cx, p, deferred))
    # the next level's zeroed histograms (at most 2 open nodes per open node) are queued before
    # the host waits for its counts, so the fill runs while the host sizes that level
    pre_hist = _runner_prologue(cx, p, inp) if p.driver is _Driver.RUNNER else _python_prologue(cx, p, inp)
    if p.compact:
        shards.sample_compact(cx.C, 0, cx.seed, cx.tree, cx.st.open[0][:1], int(Q.num_features), int(params.feat_k),
                              Q.fid_orig)
        yield cx.st.record_event(cx.stream)
    prev, ev, counted = (None, None), None, False       # (the previous level's histograms and row map)
    for d in range(params.max_depth):
        if d > 0:
            if on_first_wait is not None:
                on_first_wait()
                on_first_wait = None
            yield ev
        lv = _open_level(cx, p, d)
        if lv is None:
            break
        smp = _level_sample(cx, p, lv)
        bufs = None
        if p.dp:
            bufs = yield CollStep("alloc", rows=lv.n_build, Bs=smp.Bs, n_open=lv.n_open,
                                  totals=ws.totals if d == 0 else None,
                                  sub_rows=0 if (p.build_all or d == 0) else lv.n_build)
        out = _hist_out(cx, p, lv, smp, bufs, pre_hist)
        with tracing.span("tree.hist"):
            rg = ws.rowgroups() if (not p.build_all and p.np_ == 4) else None
            _level_hist(cx, p, lv, smp, out, bufs, rg, counted)
        if p.dp:
            yield CollStep("rs")                  # (the batch's reduce-scatter, LevelBatcher.serve)
        hist, row_of = _level_rows(cx, p, lv, out, bufs, prev)
        with tracing.span("tree.split"):
            packed = _split_search(cx, p, lv, smp, hist, bufs, row_of)
            if p.dp:
                # [S, n_open, 5] (the batch's all-gather): the plan takes the best over shards per
                # node (ties to the lowest shard = the lowest feature)
                packed = yield CollStep("ag")
        if p.runner is not None:
            ev, pre_hist, counted = _runner_plan_partition(cx, p, lv, smp, hist, packed, prev[0], rg)
        else:
            ev, pre_hist = _python_plan_partition(cx, p, lv, packed)
        prev = (hist, row_of)
    if on_first_wait is not None:          # (a one-level tree) the previous table first
        on_first_wait()
    return (yield from _read_tree(cx, p, deferred))


class _Done:
    def synchronize(self):
        pass

    def query(self) -> bool:
        return True


def _weight(st, mode) -> int:
    return int(st[1]) if mode == 0 else int(st[0] + st[1])


def _partition(C, Q: Quantized, ws: Workspace, default_child: np.ndarray, splits: list, chunk: int = 1 << 16,
               row_node: Optional[torch.Tensor] = None):
    """Rows -> children (K-13): every row of a split node moves to the default child, then one pass
    over the split columns moves the rows present in them whose bin falls on the other side."""
    hs = _partition_stage(Q, ws.staging, default_child, splits, chunk)
    up = ws.staging.upload()
    _partition_launch(C, Q, up, hs, ws.row_node if row_node is None else row_node)


def _partition_stage(Q: Quantized, stg, default_child: np.ndarray, splits: list, chunk: int = 1 << 16) -> tuple:
    """Host arrays of one tree's level partition, added to ``stg`` (upload separately)."""
    colptr = Q.colptr.cpu().numpy() if not hasattr(Q, "_colptr_host") else Q._colptr_host
    Q._colptr_host = colptr
    # splits on hot features: the row pass reads the node's bin from the dense block (1 byte per
    # row, coalesced) instead of scattering the column's millions of CSC entries
    node_dense = None
    col_splits = splits
    if Q.dense is not None:
        if getattr(Q, "_hot_row", None) is None:
            Q._hot_row = np.full(Q.Fa, -1, dtype=np.int32)
            Q._hot_row[Q.hot] = np.arange(len(Q.hot), dtype=np.int32)
        node_dense = np.full((len(default_child), 4), -1, dtype=np.int32)
        col_splits = []
        for sp in splits:
            fid, dflt, other, b, left_default, n = sp
            hr = int(Q._hot_row[fid])
            if hr >= 0:
                node_dense[n] = (hr, b, dflt if left_default else other, other if left_default else dflt)
            else:
                col_splits.append(sp)
    splits = col_splits
    starts, ends, item_split = [], [], []
    for si, sp in enumerate(splits):
        a, b = int(colptr[sp[0]]), int(colptr[sp[0] + 1])
        for s in range(a, b, chunk):
            starts.append(s)
            ends.append(min(b, s + chunk))
            item_split.append(si)
    hs = [stg.add(default_child), stg.add(np.array(starts, dtype=np.int64)), stg.add(np.array(ends, dtype=np.int64)),
          stg.add(np.array(item_split, dtype=np.int32))]
    hs += [stg.add(np.array([sp[k] for sp in splits], dtype=np.int32)) for k in (1, 2, 3, 4)]
    h_nd = stg.add(node_dense) if node_dense is not None else None
    return hs, h_nd


def _partition_launch(C, Q: Quantized, up: list, staged: tuple, row_node: torch.Tensor) -> None:
    hs, h_nd = staged
    C.tree_partition(row_node, *(up[h] for h in hs), Q.csc_row, Q.csc_bin,
                     up[h_nd] if h_nd is not None else None, Q.dense if h_nd is not None else None)