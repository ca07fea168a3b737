// Host twins of the Naive Bayes kernels (contracts in nb.h). nb_sums is its row body on the host
// pass of fixedpoint.h (private blocks, merged: the thread count does not change a bit). nb_score
// sums in spmv's order (64 lane-strided partials, halving adds, then + b_c).
#include "nb.h"

namespace fdx {

template <class V>
void nb_sums_cpu(const NbSumArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  const int C = a.num_classes;
  const int64_t F = a.F;
  uint64_t tail[2 * kNbMaxClasses] = {};           // Wq [C] | cnt [C]
  // rows [lo, hi) into the block S | Wq | cnt; returns the flag
  auto rows = [&](int64_t lo, int64_t hi, uint64_t* S, uint64_t* sums) -> int64_t {
    uint64_t *Wq = sums, *cnt = sums + C;
    int64_t flag = 0;
    for (int64_t r = lo; r < hi; ++r) {
      const int c = nb_label(a.labels[r], C);
      const double w = a.weights ? a.weights[r] : 1.0;
      if (c < 0 || !nb_weight_ok(w)) { flag = 1; continue; }
      Wq[c] += (uint64_t)nb_quant(w, a.kw);
      cnt[c] += 1;
      uint64_t* row = S + (int64_t)c * F;
      for (int64_t j = a.indptr[r]; j < a.indptr[r + 1]; ++j) {
        const int32_t f = a.idx[j];
        const double x = (double)a.val[j];
        if ((uint32_t)f >= (uint32_t)a.F || !nb_value_ok(x, a.bernoulli)) { flag = 1; continue; }
        row[f] += (uint64_t)nb_quant(w * x, a.k);
      }
    }
    return flag;
  };
  if (fx_host_pass(a.rows, threads, reinterpret_cast<uint64_t*>(a.S), (int64_t)C * F, tail, 2 * C, rows)) *a.flag = 1;
  for (int c = 0; c < C; ++c) {
    reinterpret_cast<uint64_t*>(a.Wq)[c] += tail[c];
    reinterpret_cast<uint64_t*>(a.cnt)[c] += tail[C + c];
  }
}
template void nb_sums_cpu<float>(const NbSumArgs<float>&, int);
template void nb_sums_cpu<double>(const NbSumArgs<double>&, int);

template <class V>
void nb_score_cpu(const NbScoreArgs<V>& a, int threads) {
  const int C = a.num_classes;
  parallel_for(a.rows, threads, 1024, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      double p[kNbMaxClasses][kNbWave] = {};
      const int64_t s = a.indptr[r];
      for (int64_t j = s; j < a.indptr[r + 1]; ++j) {
        const int32_t f = a.idx[j];
        if ((uint32_t)f >= (uint32_t)a.F) continue;
        const double x = (double)a.val[j];
        const double* w = a.W + (int64_t)f * C;
        for (int c = 0; c < C; ++c) p[c][(j - s) & (kNbWave - 1)] += x * w[c];
      }
      for (int c = 0; c < C; ++c) a.out[r * C + c] = nb_butterfly_host(p[c]) + a.b[c];
    }
  });
}
template void nb_score_cpu<float>(const NbScoreArgs<float>&, int);
template void nb_score_cpu<double>(const NbScoreArgs<double>&, int);

}  // namespace fdx
