// Host twins of the Naive Bayes kernels (contracts in nb.h). nb_sums gives every thread a private
// int64 table over a range of rows and merges the tables: the sums are integers, so the thread
// count does not change a bit. nb_score sums in spmv's order (64 lane-strided partials, halving
// adds, then + b_c).
#include <algorithm>
#include <atomic>
#include <vector>

#include "nb.h"
#include "parallel_for.h"

namespace fdx {

template <class V>
void nb_sums_cpu(const NbSumArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  const int C = a.num_classes;
  const int64_t F = a.F, width = (int64_t)C * F + 2 * C;
  int T = threads <= 0 ? HostPool::get().size() : threads;
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, a.rows / 256));
  // thread 0 adds into the outputs themselves
  std::vector<std::vector<uint64_t>> priv(T > 1 ? T - 1 : 0);
  std::atomic<int> bad{0};
  const int64_t per = (a.rows + T - 1) / T;
  parallel_for(T, T, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      uint64_t *S, *Wq, *cnt;
      if (t == 0) {
        S = reinterpret_cast<uint64_t*>(a.S);
        Wq = reinterpret_cast<uint64_t*>(a.Wq);
        cnt = reinterpret_cast<uint64_t*>(a.cnt);
      } else {
        priv[t - 1].assign((size_t)width, 0);
        S = priv[t - 1].data();
        Wq = S + (int64_t)C * F;
        cnt = Wq + C;
      }
      bool flag = false;
      const int64_t r1 = std::min(a.rows, (t + 1) * per);
      for (int64_t r = t * per; r < r1; ++r) {
        const int c = nb_label(a.labels[r], C);
        const double w = a.weights ? a.weights[r] : 1.0;
        if (c < 0 || !nb_weight_ok(w)) { flag = true; continue; }
        Wq[c] += (uint64_t)nb_quant(w, a.kw);
        cnt[c] += 1;
        uint64_t* row = S + (int64_t)c * F;
        for (int64_t j = a.indptr[r]; j < a.indptr[r + 1]; ++j) {
          const int32_t f = a.idx[j];
          const double x = (double)a.val[j];
          if ((uint32_t)f >= (uint32_t)a.F || !nb_value_ok(x, a.bernoulli)) { flag = true; continue; }
          row[f] += (uint64_t)nb_quant(w * x, a.k);
        }
      }
      if (flag) bad.store(1, std::memory_order_relaxed);
    }
  });
  uint64_t* out = reinterpret_cast<uint64_t*>(a.S);
  if (T > 1)
    parallel_for((int64_t)C * F, threads, 1 << 14, [&](int64_t lo, int64_t hi) {
      for (const auto& p : priv)
        for (int64_t i = lo; i < hi; ++i) out[i] += p[i];
    });
  for (const auto& p : priv)
    for (int c = 0; c < C; ++c) {
      reinterpret_cast<uint64_t*>(a.Wq)[c] += p[(int64_t)C * F + c];
      reinterpret_cast<uint64_t*>(a.cnt)[c] += p[(int64_t)C * F + C + c];
    }
  if (bad.load()) *a.flag = 1;
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
