// Batched top-k cosine retrieval over a CSR corpus: descriptors and the term functions shared by
// sim_kernels.hip and sim_cpu.cpp, so both sides execute the same operations (fp contraction is
// off in both). Three ops:
//   sim_norms   norm[r] = sqrt(sum val^2) of every row, in spmv's order (lane-strided partials of
//               64 lanes, then the xor butterfly)
//   sim_topk    per (chunk of corpus rows, tile of queries): dot(r, q) in spmv's order over row r's
//               entries (operand 0.0 where the query lacks the feature), sim = dot / max(norm qn,
//               1e-12), and the chunk's best k per query by (sim descending, row ascending)
//   sim_merge   per query: the best k of all chunks' candidates, sorted by rank
// The ranking is a total order over exact values, so the result depends on (corpus, queries, k)
// alone: not on the chunk size, the queries per pass, the grid or the host threads. No kernel uses
// an atomic on global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace fdx {

constexpr int kSimWave = 64;
constexpr int kSimBlock = 256;                            // lanes of a workgroup of sim_topk / sim_merge
constexpr int kSimWaves = kSimBlock / kSimWave;
constexpr int kSimKMax = 16;                              // kSimWaves * kSimKMax = one wave of merge slots
constexpr int kSimQueryCap = 1024;                        // distinct terms of a query held in LDS
constexpr int kSimChunkRows = 256;                        // default corpus rows per workgroup
constexpr int kSimQueriesPerPass = 4;                     // default (and largest) query tile
constexpr int64_t kSimMaxChunkRows = 1 << 20;
static_assert(kSimWaves * kSimKMax == kSimWave, "the workgroup merge ranks one candidate per lane");

// ---------------------------------------------------------------- term functions
// one multiply, one max, one divide
FDX_HD double sim_value(double dot, double norm, double qn) {
  const double d = norm * qn;
  return dot / (d > 1e-12 ? d : 1e-12);
}

// rank order: larger similarity first (compared as numbers), then the smaller row
FDX_HD bool sim_better(double sa, int64_t ra, double sb, int64_t rb) {
  return sa > sb || (sa == sb && ra < rb);
}

// exact lookup in a query's ascending feature ids; 0.0 when absent
FDX_HD double sim_lookup(const int32_t* qi, const double* qv, int len, int32_t f) {
  int lo = 0, hi = len - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t k = qi[mid];
    if (k == f) return qv[mid];
    if (k < f) lo = mid + 1; else hi = mid - 1;
  }
  return 0.0;
}

// empty slot of a best-k list: loses against every real candidate
constexpr int64_t kSimNoRow = -1;
FDX_HD double sim_no_value() { return -INFINITY; }

// insert (s, r) into a list of k entries sorted by rank; `r` ascends over the calls of one list or
// not, the order is total either way. Empty slots hold (sim_no_value(), row_empty).
template <class R>
FDX_HD void sim_insert(double* bs, R* br, int k, double s, R r, R row_empty) {
  auto better = [&](int p) {
    return br[p] == row_empty ? s > sim_no_value() : sim_better(s, (int64_t)r, bs[p], (int64_t)br[p]);
  };
  if (!better(k - 1)) return;
  int p = k - 1;
  while (p > 0 && better(p - 1)) {
    bs[p] = bs[p - 1];
    br[p] = br[p - 1];
    --p;
  }
  bs[p] = s;
  br[p] = r;
}

// host side of the 64-lane sum (lane 0 of the xor butterfly)
inline double sim_butterfly_host(double* p) {
  for (int o = kSimWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
  return p[0];
}

// slots of a query's lookup table: the power of two >= the call's longest query (and >= one wave)
inline int sim_table_cap(int64_t max_len) {
  int cap = kSimWave;
  while (cap < max_len && cap < kSimQueryCap) cap <<= 1;
  return cap;
}
inline size_t sim_table_bytes(int table_cap) {
  return (size_t)kSimQueriesPerPass * table_cap * (sizeof(double) + sizeof(int32_t));
}

inline int64_t sim_chunks(int64_t rows, int64_t chunk_rows) { return (rows + chunk_rows - 1) / chunk_rows; }

// ---------------------------------------------------------------- descriptors
template <class V>
struct SimNormArgs {
  const int64_t* indptr;   // [rows + 1]
  const V* val;
  int64_t rows;
  double* norms;           // [rows]
};

template <class V>
struct SimTopkArgs {
  const int64_t* indptr;     // [rows + 1] corpus CSR (ids ascending and distinct within a row)
  const int32_t* idx;
  const V* val;
  const double* norms;       // [rows]
  int64_t rows;
  const int64_t* q_indptr;   // [queries + 1] (every query holds <= kSimQueryCap distinct ids, any order)
  const int32_t* q_idx;
  const double* q_val;
  const double* q_norms;     // [queries]
  int64_t queries;
  int k;                     // 1 .. kSimKMax
  int chunk_rows;            // 1 .. kSimMaxChunkRows
  int queries_per_pass;      // 1 .. kSimQueriesPerPass
  int table_cap;             // device: slots of a query's LDS table, sim_table_cap(longest query)
  int64_t chunks;            // sim_chunks(rows, chunk_rows)
  double* cand_sims;         // [queries, chunks, k] sorted by rank within a (query, chunk)
  int64_t* cand_rows;        // [queries, chunks, k] kSimNoRow = no candidate
};

struct SimMergeArgs {
  const double* cand_sims;   // [queries, cands]
  const int64_t* cand_rows;
  int64_t queries, cands;
  int k, k_out;              // k_out = min(k, rows) <= cands
  double* sims;              // [queries, k_out]
  int64_t* rows;             // [queries, k_out]
};

template <class V> void launch_sim_norms(const SimNormArgs<V>& a, hipStream_t stream);
template <class V> void sim_norms_cpu(const SimNormArgs<V>& a, int threads);
template <class V> void launch_sim_topk(const SimTopkArgs<V>& a, hipStream_t stream);
template <class V> void sim_topk_cpu(const SimTopkArgs<V>& a, int threads);
void launch_sim_merge(const SimMergeArgs& a, hipStream_t stream);
void sim_merge_cpu(const SimMergeArgs& a, int threads);

}  // namespace fdx
