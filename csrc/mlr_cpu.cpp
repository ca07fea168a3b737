// Host twin of the multinomial logistic regression kernel (contract in mlr.h). Every thread owns a
// range of rows and a private int64 block, and the blocks are merged: the sums are integers, so the
// thread count does not change a bit. Margins are summed in nb_score's order (64 lane-strided
// partials, halving adds, then + b_c); the row terms are mlr_row_terms, as on the device.
#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <vector>

#include "mlr.h"
#include "parallel_for.h"

namespace fdx {

namespace {

// rows [lo, hi) into the block G | gb | loss; returns the flag bits
template <class V, int C>
int64_t mlr_rows(const MlrArgs<V>& a, int64_t lo, int64_t hi, uint64_t* G, uint64_t* gb, uint64_t* lossq) {
  int64_t flag = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const int y = nb_label(a.labels[r], C);
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = y < 0 || !mlr_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double p[C][kNbWave] = {};
    for (int64_t j = s; j < e; ++j) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      bad_row |= !mlr_value_ok(x);
      const double* xs = a.XS + (int64_t)f * C;
      for (int c = 0; c < C; ++c) p[c][(j - s) & (kNbWave - 1)] += x * xs[c];
    }
    double m[C], res[C];
    for (int c = 0; c < C; ++c) m[c] = nb_butterfly_host(p[c]) + a.b[c];
    double loss = 0.0;
    if (bad_row) {
      flag |= kMlrFlagBadInput;
      for (int c = 0; c < C; ++c) res[c] = 0.0;
    } else {
      bool clamped;
      loss = mlr_row_terms<C>(m, y, w, res, clamped);
      if (clamped) flag |= kMlrFlagClamped;
      *lossq += (uint64_t)nb_quant(w * loss, a.kl);
      for (int c = 0; c < C; ++c) gb[c] += (uint64_t)nb_quant(res[c], a.k);
    }
    if (a.margin)
      for (int c = 0; c < C; ++c) a.margin[r * C + c] = m[c];
    if (a.R)
      for (int c = 0; c < C; ++c) a.R[r * C + c] = res[c];
    if (a.loss_row) a.loss_row[r] = loss;
    if (bad_row) continue;
    for (int64_t j = s; j < e; ++j) {
      const double x = (double)a.val[j];
      uint64_t* dst = G + (int64_t)a.idx[j] * C;
      for (int c = 0; c < C; ++c) dst[c] += (uint64_t)nb_quant(x * res[c], a.k);
    }
  }
  return flag;
}

template <class V, int C>
void mlr_eval_c(const MlrArgs<V>& a, int threads) {
  const int64_t width = (int64_t)C * a.F;
  int T = threads <= 0 ? HostPool::get().size() : threads;
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, a.rows / 256));
  // thread 0 adds into the outputs themselves
  std::vector<std::vector<uint64_t>> priv(T > 1 ? T - 1 : 0);
  std::atomic<int64_t> flags{0};
  const int64_t per = (a.rows + T - 1) / T;
  parallel_for(T, T, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      uint64_t *G, *gb, *lossq;
      if (t == 0) {
        G = reinterpret_cast<uint64_t*>(a.Gq);
        gb = reinterpret_cast<uint64_t*>(a.gbq);
        lossq = reinterpret_cast<uint64_t*>(a.lossq);
      } else {
        priv[t - 1].assign((size_t)width + C + 1, 0);
        G = priv[t - 1].data();
        gb = G + width;
        lossq = gb + C;
      }
      const int64_t f = mlr_rows<V, C>(a, std::min(a.rows, t * per), std::min(a.rows, (t + 1) * per), G, gb, lossq);
      if (f) flags.fetch_or(f, std::memory_order_relaxed);
    }
  });
  uint64_t* out = reinterpret_cast<uint64_t*>(a.Gq);
  if (T > 1)
    parallel_for(width, threads, 1 << 14, [&](int64_t lo, int64_t hi) {
      for (const auto& p : priv)
        for (int64_t i = lo; i < hi; ++i) out[i] += p[i];
    });
  for (const auto& p : priv) {
    for (int c = 0; c < C; ++c) reinterpret_cast<uint64_t*>(a.gbq)[c] += p[width + c];
    *reinterpret_cast<uint64_t*>(a.lossq) += p[width + C];
  }
  *a.flag |= flags.load();
}

}  // namespace

template <class V>
void mlr_eval_cpu(const MlrArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  switch (a.num_classes) {
    case 2: mlr_eval_c<V, 2>(a, threads); break;
    case 3: mlr_eval_c<V, 3>(a, threads); break;
    case 4: mlr_eval_c<V, 4>(a, threads); break;
    case 5: mlr_eval_c<V, 5>(a, threads); break;
    case 6: mlr_eval_c<V, 6>(a, threads); break;
    case 7: mlr_eval_c<V, 7>(a, threads); break;
    case 8: mlr_eval_c<V, 8>(a, threads); break;
    default: throw std::runtime_error("fdx mlr_eval: classes out of range");
  }
}
template void mlr_eval_cpu<float>(const MlrArgs<float>&, int);
template void mlr_eval_cpu<double>(const MlrArgs<double>&, int);

}  // namespace fdx
