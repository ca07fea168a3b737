// Batched top-k cosine retrieval for gfx950 (contract and descriptors: sim.h).
//
// sim_topk: a workgroup of four waves takes one chunk of consecutive corpus rows and one tile of up
// to kSimQueriesPerPass queries. The tile's queries sit in LDS as ascending (feature id, value)
// arrays, read-only after the build (a query stored out of order is sorted in LDS first). The
// arrays are dynamic LDS of table_cap slots a query, the power of two that holds the call's
// longest query: 12 KiB a query at the 1024-term capacity (3 workgroups a CU), 1.5 KiB for
// 128-term dialogues, where the registers, not the LDS, bound the occupancy. Every wave streams
// rows of the chunk: a row's entries are read once, coalesced, each entry is looked up in every
// query of the tile by binary search, and the per-query dots accumulate in spmv_kernel's order
// (lane-strided partials, xor butterfly). Lane q of the wave then keeps query q's best k of the
// wave's rows in LDS; most rows fail the first compare against the current k-th. The workgroup's 4 x 16 list slots are ranked by one wave per
// query, one slot per lane, and the chunk's k candidates go to global memory with plain stores.
// Workgroups of the same chunk (different tiles) are adjacent in the grid, so the chunk's rows are
// served from cache to all but the first of them.
//
// sim_merge: one workgroup per query selects the best k of all chunks' candidates, one rank per
// round (the best candidate strictly behind the previous round's).
#include <stdexcept>

#include "sim.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kSimWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kSimWave);
  return v;
}

template <class V>
__global__ __launch_bounds__(kSimBlock) void sim_norms_kernel(SimNormArgs<V> a) {
  const int lane = threadIdx.x & (kSimWave - 1);
  const int64_t r = (int64_t)blockIdx.x * kSimWaves + threadIdx.x / kSimWave;
  if (r >= a.rows) return;
  double part = 0.0;
  for (int64_t j = a.indptr[r] + lane; j < a.indptr[r + 1]; j += kSimWave) {
    const double v = (double)a.val[j];
    part += v * v;
  }
  part = wave_sum(part);
  if (lane == 0) a.norms[r] = sqrt(part);
}

constexpr int32_t kPadKey = 0x7fffffff;   // sorts behind every feature id

template <class V>
__global__ __launch_bounds__(kSimBlock) void sim_topk_kernel(SimTopkArgs<V> a) {
  // kSimQueriesPerPass tables of a.table_cap (id, value) slots: the values first, then the ids
  extern __shared__ double sim_tables[];
  const int cap = a.table_cap;
  auto q_val = [&](int q) { return sim_tables + (size_t)q * cap; };
  auto q_idx = [&](int q) { return reinterpret_cast<int32_t*>(sim_tables + (size_t)kSimQueriesPerPass * cap) + (size_t)q * cap; };
  __shared__ double best_sim[kSimWaves][kSimQueriesPerPass][kSimKMax];
  __shared__ int32_t best_row[kSimWaves][kSimQueriesPerPass][kSimKMax];   // row within the chunk, -1 = empty
  __shared__ int q_len[kSimQueriesPerPass];
  __shared__ int q_unsorted[kSimQueriesPerPass];
  __shared__ double q_norm[kSimQueriesPerPass];

  const int tid = threadIdx.x, lane = tid & (kSimWave - 1), wave = tid / kSimWave;
  const int qpp = a.queries_per_pass;
  const int64_t tiles = (a.queries + qpp - 1) / qpp;
  const int64_t chunk = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x % tiles;
  const int64_t q0 = tile * qpp;
  const int nq = (int)(a.queries - q0 < qpp ? a.queries - q0 : qpp);
  const int64_t r0 = chunk * a.chunk_rows;
  const int nrows = (int)(a.rows - r0 < a.chunk_rows ? a.rows - r0 : a.chunk_rows);
  const int k = a.k;

  // ---- build the tile's tables
  if (tid < kSimQueriesPerPass) {
    int len = 0;
    if (tid < nq) {
      const int64_t l = a.q_indptr[q0 + tid + 1] - a.q_indptr[q0 + tid];
      len = (int)(l < 0 ? 0 : (l > cap ? cap : l));   // the launcher sizes the tables for the longest query
      q_norm[tid] = a.q_norms[q0 + tid];
    }
    q_len[tid] = len;
    q_unsorted[tid] = 0;
  }
  for (int i = tid; i < kSimWaves * kSimQueriesPerPass * kSimKMax; i += kSimBlock) {
    (&best_sim[0][0][0])[i] = sim_no_value();
    (&best_row[0][0][0])[i] = -1;
  }
  __syncthreads();
  for (int q = 0; q < nq; ++q) {
    const int len = q_len[q];
    const int64_t s = a.q_indptr[q0 + q];
    for (int i = tid; i < len; i += kSimBlock) {
      const int32_t f = a.q_idx[s + i];
      q_idx(q)[i] = f;
      q_val(q)[i] = a.q_val[s + i];
      if (i > 0 && a.q_idx[s + i - 1] >= f) q_unsorted[q] = 1;   // every writer stores the same value
    }
  }
  __syncthreads();
  for (int q = 0; q < nq; ++q) {
    if (!q_unsorted[q]) continue;                 // uniform over the workgroup
    const int len = q_len[q];
    int n2 = 1;
    while (n2 < len) n2 <<= 1;                    // <= table_cap, a power of two
    for (int i = len + tid; i < n2; i += kSimBlock) { q_idx(q)[i] = kPadKey; q_val(q)[i] = 0.0; }
    __syncthreads();
    int32_t* const ki = q_idx(q);
    double* const kv = q_val(q);
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < n2; i += kSimBlock) {
          const int j = i ^ stride;
          if (j > i) {
            const bool up = (i & size) == 0;
            const int32_t x = ki[i], y = ki[j];
            if ((x > y) == up) {
              ki[i] = y; ki[j] = x;
              const double t = kv[i]; kv[i] = kv[j]; kv[j] = t;
            }
          }
        }
        __syncthreads();
      }
  }

  // ---- stream the chunk's rows: wave w takes rows w, w + 4, ... (ascending, so ties keep the smaller row)
  for (int lr = wave; lr < nrows; lr += kSimWaves) {
    const int64_t r = r0 + lr;
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double part[kSimQueriesPerPass];
#pragma unroll
    for (int q = 0; q < kSimQueriesPerPass; ++q) part[q] = 0.0;
    for (int64_t j = s + lane; j < e; j += kSimWave) {
      const int32_t f = a.idx[j];
      const double v = (double)a.val[j];
#pragma unroll
      for (int q = 0; q < kSimQueriesPerPass; ++q)
        if (q < nq) part[q] += v * sim_lookup(q_idx(q), q_val(q), q_len[q], f);
    }
    double mine = 0.0;
#pragma unroll
    for (int q = 0; q < kSimQueriesPerPass; ++q) {
      if (q < nq) {
        const double d = wave_sum(part[q]);      // every lane holds the same bits
        if (lane == q) mine = d;
      }
    }
    if (lane < nq) {
      const double sim = sim_value(mine, a.norms[r], q_norm[lane]);
      sim_insert<int32_t>(best_sim[wave][lane], best_row[wave][lane], k, sim, (int32_t)lr, -1);
    }
  }
  __syncthreads();

  // ---- merge: wave q ranks query q's 64 list slots (wave l / 16, slot l % 16), one per lane
  for (int q = wave; q < nq; q += kSimWaves) {
    const int w = lane / kSimKMax, sl = lane % kSimKMax;
    const bool live = sl < k && best_row[w][q][sl] >= 0;
    const double ms = live ? best_sim[w][q][sl] : sim_no_value();
    const int32_t mr = live ? best_row[w][q][sl] : -1;
    int rank = 0;
    for (int j = 0; j < kSimWave; ++j) {
      const int wj = j / kSimKMax, sj = j % kSimKMax;
      const bool lj = sj < k && best_row[wj][q][sj] >= 0;
      if (!lj) { rank += (!live && j < lane) ? 1 : 0; continue; }    // empty slots rank last, by lane
      if (!live || sim_better(best_sim[wj][q][sj], best_row[wj][q][sj], ms, mr)) ++rank;
    }
    if (rank < k) {
      const int64_t o = ((q0 + q) * a.chunks + chunk) * k + rank;
      a.cand_sims[o] = ms;
      a.cand_rows[o] = live ? r0 + mr : kSimNoRow;
    }
  }
}

__global__ __launch_bounds__(kSimBlock) void sim_merge_kernel(SimMergeArgs a) {
  __shared__ double w_sim[kSimWaves];
  __shared__ int64_t w_row[kSimWaves];
  __shared__ double prev_sim;
  __shared__ int64_t prev_row;
  const int tid = threadIdx.x, lane = tid & (kSimWave - 1), wave = tid / kSimWave;
  const int64_t q = blockIdx.x;
  const double* cs = a.cand_sims + q * a.cands;
  const int64_t* cr = a.cand_rows + q * a.cands;
  for (int round = 0; round < a.k_out; ++round) {
    const double ps = round ? prev_sim : 0.0;
    const int64_t pr = round ? prev_row : kSimNoRow;
    double bs = sim_no_value();
    int64_t br = kSimNoRow;
    for (int64_t i = tid; i < a.cands; i += kSimBlock) {
      const int64_t r = cr[i];
      if (r < 0) continue;
      const double s = cs[i];
      if (round && !sim_better(ps, pr, s, r)) continue;        // not strictly behind the previous pick
      if (br < 0 ? s > sim_no_value() : sim_better(s, r, bs, br)) { bs = s; br = r; }
    }
#pragma unroll
    for (int o = kSimWave / 2; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, kSimWave);
      const int64_t orow = __shfl_xor(br, o, kSimWave);
      if (orow >= 0 && (br < 0 || sim_better(os, orow, bs, br))) { bs = os; br = orow; }
    }
    if (lane == 0) { w_sim[wave] = bs; w_row[wave] = br; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kSimWaves; ++w)
        if (w_row[w] >= 0 && (br < 0 || sim_better(w_sim[w], w_row[w], bs, br))) { bs = w_sim[w]; br = w_row[w]; }
      prev_sim = bs;
      prev_row = br;
      a.sims[q * a.k_out + round] = bs;
      a.rows[q * a.k_out + round] = br;
    }
    __syncthreads();
  }
}

}  // namespace

template <class V>
void launch_sim_norms(const SimNormArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  const unsigned grid = (unsigned)((a.rows + kSimWaves - 1) / kSimWaves);
  hipLaunchKernelGGL(sim_norms_kernel<V>, dim3(grid), dim3(kSimBlock), 0, stream, a);
}
template void launch_sim_norms<float>(const SimNormArgs<float>&, hipStream_t);
template void launch_sim_norms<double>(const SimNormArgs<double>&, hipStream_t);

template <class V>
void launch_sim_topk(const SimTopkArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0 || a.queries <= 0) return;
  const int64_t tiles = (a.queries + a.queries_per_pass - 1) / a.queries_per_pass;
  if (a.table_cap < kSimWave || a.table_cap > kSimQueryCap || (a.table_cap & (a.table_cap - 1)))
    throw std::runtime_error("fdx sim_topk: table_cap must be a power of two in 64 .. query_cap");
  hipLaunchKernelGGL(sim_topk_kernel<V>, dim3((unsigned)(a.chunks * tiles)), dim3(kSimBlock),
                     sim_table_bytes(a.table_cap), stream, a);
}
template void launch_sim_topk<float>(const SimTopkArgs<float>&, hipStream_t);
template void launch_sim_topk<double>(const SimTopkArgs<double>&, hipStream_t);

void launch_sim_merge(const SimMergeArgs& a, hipStream_t stream) {
  if (a.queries <= 0 || a.k_out <= 0) return;
  hipLaunchKernelGGL(sim_merge_kernel, dim3((unsigned)a.queries), dim3(kSimBlock), 0, stream, a);
}

}  // namespace fdx
