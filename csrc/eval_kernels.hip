// Validation monitoring of the GBDT trainer for gfx950, wave64 (descriptors and per-element code:
// eval.h; host twins: eval_cpu.cpp).
//
// tree_eval_update: one wave per validation row, kEvalRowsPerGroup rows per workgroup at a time, at
//   most kEvalMaxGroups workgroups whose waves stride over the rows. Each workgroup first resolves
//   the node table into LDS (original feature, threshold, children, leaf value per node). The row's
//   first kEvalWaveLoad (index, value) pairs are loaded once, coalesced, one per lane; at every tree
//   level the wave finds the split feature with one ballot and reads its value from the owning
//   lane (no per-lane binary search of dependent loads). Longer rows continue with further
//   wave-loads from memory, stopping at the first one whose indices pass the feature (sorted rows).
//   The node walk is wave-uniform: every lane follows the same row.
// eval_sums: exact int64 sums -- a wave shuffle reduction, an LDS reduction per workgroup and one
//   integer atomic per workgroup and sum (integers: no dependence on the grid or the order).
// eval_auc: keys + labels -> hipCUB radix sort -> three passes over tiles of kEvalAucTile sorted
//   elements. With neg[i] = negatives before sorted position i (non-decreasing), a positive in the
//   run of equal keys [s, e) contributes neg[s] + neg[e] to U2: neg[s] is the max-scan of neg over
//   run heads, neg[e] the reverse min-scan of neg[i + 1] over run tails; both carry across tiles
//   through a tile-level scan, so no run is tracked across workgroups.
// No float atomics, no waiting between workgroups.
#include <hipcub/hipcub.hpp>

#include "eval.h"
#include "ops.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {
constexpr int kWave = kEvalWave;
constexpr int kBlock = kEvalReduceBlock;
constexpr int kTile = kEvalAucTile;
static_assert(kTile == kBlock, "one sorted element per lane");
static_assert(kEvalRowsPerGroup * kWave == 256, "tree_eval_update workgroup");
constexpr int64_t kNoTail = INT64_MAX;

// One node of the tree as the walk needs it, resolved once per workgroup into LDS: the walk of a
// row then costs one LDS read per level instead of a chain of dependent global loads (node ->
// active feature -> original feature / threshold offset -> threshold).
struct EvalNode {
  double thr;
  double value;       // eval_leaf of the node
  int32_t fid;        // original feature of an inner node, -1: the walk ends here
  int32_t left, right;
  int32_t pad;
};

template <class V>
__global__ __launch_bounds__(256) void tree_eval_update_kernel(TreeEvalArgs<V> a) {
  extern __shared__ EvalNode nodes[];
  const EvalTree& t = a.t;
  for (int32_t n = threadIdx.x; n < t.max_nodes; n += 256) {
    EvalNode nd;
    nd.thr = 0.0;
    nd.value = eval_leaf(t, n);
    nd.fid = -1;
    nd.left = t.left[n];
    nd.right = t.right[n];
    nd.pad = 0;
    if (eval_is_inner(t, n)) {
      const int64_t j = t.boff[t.feat[n]] + t.bin[n];
      if (j >= 0 && j < t.TB) {
        nd.thr = t.thresholds[j];
        nd.fid = (int32_t)t.fid_orig[t.feat[n]];
      }
    }
    nodes[n] = nd;
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * kEvalRowsPerGroup;
  // (whole waves: r is wave-uniform, so every branch below is taken by all 64 lanes or none)
  for (int64_t r = (int64_t)blockIdx.x * kEvalRowsPerGroup + threadIdx.x / kWave; r < a.rows; r += stride) {
    const int64_t b = a.indptr[r], e = a.indptr[r + 1];
    const bool have = b + lane < e;
    const int32_t my_idx = have ? a.idx[b + lane] : INT32_MAX;
    const double my_val = have ? (double)a.val[b + lane] : 0.0;
    int32_t n = 0;
    for (int guard = 0; guard < kEvalMaxWalk; ++guard) {
      const EvalNode nd = nodes[n];
      const int32_t f = nd.fid;
      if (f < 0) break;
      double x = 0.0;
      unsigned long long hit = __ballot(my_idx == f);
      if (hit) {
        x = __shfl(my_val, __ffsll(hit) - 1, kWave);
      } else if (e - b > kEvalWaveLoad && !__ballot(my_idx > f)) {
        // (every loaded index is below f: the feature may sit in a later wave-load)
        for (int64_t base = b + kEvalWaveLoad; base < e; base += kEvalWaveLoad) {
          const bool in = base + lane < e;
          const int32_t i2 = in ? a.idx[base + lane] : INT32_MAX;
          hit = __ballot(i2 == f);
          if (hit) {
            const double v2 = in ? (double)a.val[base + lane] : 0.0;
            x = __shfl(v2, __ffsll(hit) - 1, kWave);
            break;
          }
          if (__ballot(i2 > f)) break;
        }
      }
      const int32_t c = x < nd.thr ? nd.left : nd.right;
      if (c < 0 || c >= t.max_nodes) break;          // (a malformed table ends the walk, as eval_next)
      n = c;
    }
    if (lane == 0) a.margin[r] += nodes[n].value;
  }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

// the workgroup's sum of three int64 per lane, added to out[0..3) by one lane
__device__ __forceinline__ void block_add3(int64_t l, int64_t e, int64_t w, int64_t* out) {
  __shared__ int64_t part[kBlock / kWave][3];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  l = wave_sum(l);
  e = wave_sum(e);
  w = wave_sum(w);
  if (lane == 0) {
    part[wv][0] = l;
    part[wv][1] = e;
    part[wv][2] = w;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) s += part[k][threadIdx.x];
    if (s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + threadIdx.x), (unsigned long long)s);
  }
}

__global__ __launch_bounds__(kBlock) void eval_sums_kernel(EvalSumArgs a) {
  int64_t l = 0, e = 0, w = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    const EvalTerms t = eval_terms(a.margin[i], a.label[i], a.weight ? (double)a.weight[i] : 1.0, a.scale);
    l += t.l;
    e += t.e;
    w += t.w;
  }
  block_add3(l, e, w, a.out);
}

// ---------------------------------------------------------------- AUC
__global__ __launch_bounds__(kBlock) void auc_keys_kernel(const double* __restrict__ margin,
                                                          const float* __restrict__ label, int64_t n,
                                                          uint64_t* __restrict__ keys, uint8_t* __restrict__ labels) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    keys[i] = eval_auc_key(margin[i]);
    labels[i] = label[i] > 0.5f ? 1 : 0;
  }
}

// tiles layout [4][nt]: negatives of the tile | negatives before the tile | max neg[] over the
// tile's run heads (-1: none) | min neg[i + 1] over its run tails (kNoTail: none); the carries
// pass overwrites rows 2 and 3 with their exclusive max / reverse min scans
using BlockScanT = hipcub::BlockScan<int64_t, kBlock>;
using BlockReduceT = hipcub::BlockReduce<int64_t, kBlock>;

__global__ __launch_bounds__(kBlock) void auc_tile_neg_kernel(const uint8_t* __restrict__ labels, int64_t n,
                                                              int64_t* __restrict__ tiles) {
  __shared__ typename BlockReduceT::TempStorage tmp;
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const int64_t neg = (i < n && !labels[i]) ? 1 : 0;
  const int64_t s = BlockReduceT(tmp).Sum(neg);
  if (threadIdx.x == 0) tiles[blockIdx.x] = s;
}

// one workgroup: tiles[1] = exclusive sum of tiles[0]; out = (0, P, N)
__global__ __launch_bounds__(kBlock) void auc_tile_offsets_kernel(int64_t nt, int64_t n, int64_t* __restrict__ tiles,
                                                                  int64_t* __restrict__ out) {
  __shared__ typename BlockScanT::TempStorage tmp;
  int64_t carry = 0;
  for (int64_t base = 0; base < nt; base += kBlock) {
    const int64_t t = base + threadIdx.x;
    const int64_t v = t < nt ? tiles[t] : 0;
    int64_t ex, total;
    BlockScanT(tmp).ExclusiveSum(v, ex, total);
    if (t < nt) tiles[nt + t] = carry + ex;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = 0;
    out[1] = n - carry;
    out[2] = carry;
  }
}

struct MaxOp {
  __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};
struct MinOp {
  __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a < b ? a : b; }
};

// The element of a lane: its run-head value (neg[i] where position i starts a run of equal keys,
// else -1) and run-tail value (neg[i + 1] where it ends one, else kNoTail). Positions >= n are
// neither. `neg_ex` = the lane's exclusive count of negatives inside the tile.
struct AucElem {
  int64_t head, tail;
  bool pos;
};

__device__ __forceinline__ AucElem auc_elem(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ labels,
                                            int64_t n, int64_t i, int64_t tile_off, int64_t neg_ex, int64_t neg) {
  AucElem el{-1, kNoTail, false};
  if (i < n) {
    const uint64_t k = keys[i];
    const int64_t before = tile_off + neg_ex;
    if (i == 0 || keys[i - 1] != k) el.head = before;
    if (i == n - 1 || keys[i + 1] != k) el.tail = before + neg;
    el.pos = labels[i] != 0;
  }
  return el;
}

__global__ __launch_bounds__(kBlock) void auc_tile_runs_kernel(const uint64_t* __restrict__ keys,
                                                               const uint8_t* __restrict__ labels, int64_t n,
                                                               int64_t nt, int64_t* __restrict__ tiles) {
  __shared__ typename BlockScanT::TempStorage tmp;
  __shared__ typename BlockReduceT::TempStorage rtmp;
  const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const int64_t neg = (i < n && !labels[i]) ? 1 : 0;
  int64_t neg_ex;
  BlockScanT(tmp).ExclusiveSum(neg, neg_ex);
  const AucElem el = auc_elem(keys, labels, n, i, tiles[nt + blockIdx.x], neg_ex, neg);
  const int64_t hmax = BlockReduceT(rtmp).Reduce(el.head, MaxOp());
  __syncthreads();
  const int64_t tmin = BlockReduceT(rtmp).Reduce(el.tail, MinOp());
  if (threadIdx.x == 0) {
    tiles[2 * nt + blockIdx.x] = hmax;
    tiles[3 * nt + blockIdx.x] = tmin;
  }
}

// one workgroup: row 2 -> exclusive max-scan (heads of earlier tiles), row 3 -> exclusive reverse
// min-scan (tails of later tiles), both in place
__global__ __launch_bounds__(kBlock) void auc_tile_carries_kernel(int64_t nt, int64_t* __restrict__ tiles) {
  __shared__ typename BlockScanT::TempStorage tmp;
  int64_t* hm = tiles + 2 * nt;
  int64_t* tm = tiles + 3 * nt;
  int64_t carry = -1;
  for (int64_t base = 0; base < nt; base += kBlock) {
    const int64_t t = base + threadIdx.x;
    const int64_t v = t < nt ? hm[t] : -1;
    int64_t ex, total;
    BlockScanT(tmp).ExclusiveScan(v, ex, (int64_t)-1, MaxOp(), total);
    if (t < nt) hm[t] = carry > ex ? carry : ex;
    carry = carry > total ? carry : total;
    __syncthreads();
  }
  carry = kNoTail;
  for (int64_t base = 0; base < nt; base += kBlock) {
    const int64_t t = nt - 1 - (base + threadIdx.x);       // (lane order = reverse tile order)
    const int64_t v = t >= 0 ? tm[t] : kNoTail;
    int64_t ex, total;
    BlockScanT(tmp).ExclusiveScan(v, ex, kNoTail, MinOp(), total);
    if (t >= 0) tm[t] = carry < ex ? carry : ex;
    carry = carry < total ? carry : total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void auc_tile_sum_kernel(const uint64_t* __restrict__ keys,
                                                              const uint8_t* __restrict__ labels, int64_t n, int64_t nt,
                                                              const int64_t* __restrict__ tiles, int64_t* __restrict__ out) {
  __shared__ typename BlockScanT::TempStorage tmp;
  __shared__ typename BlockReduceT::TempStorage rtmp;
  __shared__ int64_t tails[kTile];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kTile + tid;
  const int64_t neg = (i < n && !labels[i]) ? 1 : 0;
  int64_t neg_ex;
  BlockScanT(tmp).ExclusiveSum(neg, neg_ex);
  const AucElem el = auc_elem(keys, labels, n, i, tiles[nt + blockIdx.x], neg_ex, neg);
  __syncthreads();
  int64_t start;
  BlockScanT(tmp).InclusiveScan(el.head, start, MaxOp());
  const int64_t hc = tiles[2 * nt + blockIdx.x];
  start = start > hc ? start : hc;
  // the reverse min-scan: lane tid scans the element of lane kTile - 1 - tid
  tails[tid] = el.tail;
  __syncthreads();
  int64_t end_rev;
  BlockScanT(tmp).InclusiveScan(tails[kTile - 1 - tid], end_rev, MinOp());
  __syncthreads();
  tails[kTile - 1 - tid] = end_rev;
  __syncthreads();
  const int64_t tc = tiles[3 * nt + blockIdx.x];
  const int64_t end = tails[tid] < tc ? tails[tid] : tc;
  const int64_t u = el.pos ? start + end : 0;
  const int64_t s = BlockReduceT(rtmp).Sum(u);
  if (tid == 0 && s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)s);
}

inline unsigned grid_for(int64_t n, int64_t cap = 4096) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
}  // namespace

template <class V>
void launch_tree_eval_update(const TreeEvalArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  FDX_LANES_CHECK(a.t.max_nodes >= 1 && a.t.max_nodes <= kEvalMaxNodes);
  int64_t groups = (a.rows + kEvalRowsPerGroup - 1) / kEvalRowsPerGroup;
  if (groups > kEvalMaxGroups) groups = kEvalMaxGroups;       // (the waves stride over the rest)
  hipLaunchKernelGGL(tree_eval_update_kernel<V>, dim3((unsigned)groups), dim3(256),
                     sizeof(EvalNode) * (size_t)a.t.max_nodes, stream, a);
}
template void launch_tree_eval_update<float>(const TreeEvalArgs<float>&, hipStream_t);
template void launch_tree_eval_update<double>(const TreeEvalArgs<double>&, hipStream_t);

void launch_eval_sums(const EvalSumArgs& a, int blocks, hipStream_t stream) {
  if (a.n <= 0) return;
  const unsigned grid = blocks > 0 ? (unsigned)blocks : grid_for(a.n, 1024);
  hipLaunchKernelGGL(eval_sums_kernel, dim3(grid), dim3(kBlock), 0, stream, a);
}

int64_t eval_auc_tiles(int64_t n) { return n > 0 ? (n + kTile - 1) / kTile : 1; }

size_t eval_auc_temp_bytes(int64_t n) {
  size_t bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint8_t*)nullptr,
                                     (uint8_t*)nullptr, (size_t)(n > 0 ? n : 1), 0, 64);
  return bytes;
}

void launch_eval_auc(const double* margin, const float* label, int64_t n, const EvalAucScratch& s, int64_t* out,
                     hipStream_t stream) {
  if (n <= 0) {
    hipMemsetAsync(out, 0, 3 * sizeof(int64_t), stream);
    return;
  }
  const int64_t nt = eval_auc_tiles(n);
  FDX_LANES_CHECK(nt <= 0x7fffffffll);
  hipLaunchKernelGGL(auc_keys_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, margin, label, n, s.keys[0], s.labels[0]);
  size_t bytes = s.temp_bytes;
  hipcub::DeviceRadixSort::SortPairs(s.temp, bytes, s.keys[0], s.keys[1], s.labels[0], s.labels[1], (size_t)n, 0, 64, stream);
  const uint64_t* keys = s.keys[1];
  const uint8_t* labels = s.labels[1];
  hipLaunchKernelGGL(auc_tile_neg_kernel, dim3((unsigned)nt), dim3(kBlock), 0, stream, labels, n, s.tiles);
  hipLaunchKernelGGL(auc_tile_offsets_kernel, dim3(1), dim3(kBlock), 0, stream, nt, n, s.tiles, out);
  hipLaunchKernelGGL(auc_tile_runs_kernel, dim3((unsigned)nt), dim3(kBlock), 0, stream, keys, labels, n, nt, s.tiles);
  hipLaunchKernelGGL(auc_tile_carries_kernel, dim3(1), dim3(kBlock), 0, stream, nt, s.tiles);
  hipLaunchKernelGGL(auc_tile_sum_kernel, dim3((unsigned)nt), dim3(kBlock), 0, stream, keys, labels, n, nt, s.tiles, out);
}

}  // namespace fdx
