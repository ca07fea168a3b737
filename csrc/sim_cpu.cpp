// Host twins of the top-k cosine retrieval kernels (sim_kernels.hip): the same term functions
// (sim.h), the same summation order (64 lane-strided partials, then the butterfly's lane 0) and the
// same total order of the ranking, so the results agree with the device bit for bit.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "parallel_for.h"
#include "sim.h"

#pragma clang fp contract(off)

namespace fdx {

template <class V>
void sim_norms_cpu(const SimNormArgs<V>& a, int threads) {
  parallel_for(a.rows, threads, 1024, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      double p[kSimWave] = {0};
      const int64_t s = a.indptr[r];
      for (int64_t j = s; j < a.indptr[r + 1]; ++j) {
        const double v = (double)a.val[j];
        p[(j - s) & (kSimWave - 1)] += v * v;
      }
      a.norms[r] = std::sqrt(sim_butterfly_host(p));
    }
  });
}
template void sim_norms_cpu<float>(const SimNormArgs<float>&, int);
template void sim_norms_cpu<double>(const SimNormArgs<double>&, int);

template <class V>
void sim_topk_cpu(const SimTopkArgs<V>& a, int threads) {
  if (a.rows <= 0 || a.queries <= 0) return;
  // ascending copies of the queries (the lookup tables of the device tiles)
  std::vector<int64_t> qp(a.queries + 1, 0);
  for (int64_t q = 0; q < a.queries; ++q) {
    const int64_t l = a.q_indptr[q + 1] - a.q_indptr[q];
    qp[q + 1] = qp[q] + std::min<int64_t>(std::max<int64_t>(l, 0), kSimQueryCap);
  }
  std::vector<int32_t> qi(qp[a.queries]);
  std::vector<double> qv(qp[a.queries]);
  parallel_for(a.queries, threads, 16, [&](int64_t lo, int64_t hi) {
    std::vector<int> order;
    for (int64_t q = lo; q < hi; ++q) {
      const int len = (int)(qp[q + 1] - qp[q]);
      const int64_t s = a.q_indptr[q];
      order.resize(len);
      std::iota(order.begin(), order.end(), 0);
      std::sort(order.begin(), order.end(), [&](int x, int y) { return a.q_idx[s + x] < a.q_idx[s + y]; });
      for (int i = 0; i < len; ++i) {
        qi[qp[q] + i] = a.q_idx[s + order[i]];
        qv[qp[q] + i] = a.q_val[s + order[i]];
      }
    }
  });
  const int k = a.k;
  parallel_for(a.chunks, threads, 1, [&](int64_t lo, int64_t hi) {
    std::vector<double> bs((size_t)a.queries * k);
    std::vector<int64_t> br((size_t)a.queries * k);
    for (int64_t c = lo; c < hi; ++c) {
      std::fill(bs.begin(), bs.end(), sim_no_value());
      std::fill(br.begin(), br.end(), kSimNoRow);
      const int64_t r0 = c * a.chunk_rows, r1 = std::min(a.rows, r0 + a.chunk_rows);
      for (int64_t r = r0; r < r1; ++r) {
        const int64_t s = a.indptr[r], e = a.indptr[r + 1];
        for (int64_t q = 0; q < a.queries; ++q) {
          const int32_t* ti = qi.data() + qp[q];
          const double* tv = qv.data() + qp[q];
          const int len = (int)(qp[q + 1] - qp[q]);
          double p[kSimWave] = {0};
          for (int64_t j = s; j < e; ++j)
            p[(j - s) & (kSimWave - 1)] += (double)a.val[j] * sim_lookup(ti, tv, len, a.idx[j]);
          const double sim = sim_value(sim_butterfly_host(p), a.norms[r], a.q_norms[q]);
          sim_insert<int64_t>(bs.data() + q * k, br.data() + q * k, k, sim, r, kSimNoRow);
        }
      }
      for (int64_t q = 0; q < a.queries; ++q)
        for (int i = 0; i < k; ++i) {
          const int64_t o = (q * a.chunks + c) * k + i;
          a.cand_sims[o] = bs[q * k + i];
          a.cand_rows[o] = br[q * k + i];
        }
    }
  });
}
template void sim_topk_cpu<float>(const SimTopkArgs<float>&, int);
template void sim_topk_cpu<double>(const SimTopkArgs<double>&, int);

void sim_merge_cpu(const SimMergeArgs& a, int threads) {
  if (a.queries <= 0 || a.k_out <= 0) return;
  parallel_for(a.queries, threads, 4, [&](int64_t lo, int64_t hi) {
    std::vector<double> bs(a.k_out);
    std::vector<int64_t> br(a.k_out);
    for (int64_t q = lo; q < hi; ++q) {
      std::fill(bs.begin(), bs.end(), sim_no_value());
      std::fill(br.begin(), br.end(), kSimNoRow);
      for (int64_t i = 0; i < a.cands; ++i) {
        const int64_t r = a.cand_rows[q * a.cands + i];
        if (r >= 0) sim_insert<int64_t>(bs.data(), br.data(), a.k_out, a.cand_sims[q * a.cands + i], r, kSimNoRow);
      }
      for (int i = 0; i < a.k_out; ++i) {
        a.sims[q * a.k_out + i] = bs[i];
        a.rows[q * a.k_out + i] = br[i];
      }
    }
  });
}

}  // namespace fdx
