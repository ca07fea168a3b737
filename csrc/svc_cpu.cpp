// Host twin of the linear SVC kernel (contract in svc.h). Every thread owns a range of rows and a
// private int64 block, and the blocks are merged: the sums are integers, so the thread count does
// not change a bit. The margin is summed in spmv's order (64 lane-strided partials, halving adds,
// then + b); the row terms are svc_row_terms, as on the device, so the block equals the device's.
#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <vector>

#include "svc.h"
#include "parallel_for.h"

namespace fdx {

namespace {

// rows [lo, hi) into G and sums = (gbq, lossq, nact); returns the flag bits
template <class V>
int64_t svc_rows(const SvcArgs<V>& a, int64_t lo, int64_t hi, uint64_t* G, uint64_t* sums) {
  int64_t flag = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const double y = a.labels[r];
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !svc_label_ok(y) || !mlr_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double p[kNbWave] = {};
    for (int64_t j = s; j < e; ++j) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      bad_row |= !mlr_value_ok(x);
      p[(j - s) & (kNbWave - 1)] += x * a.xs[f];
    }
    const double m = nb_butterfly_host(p) + a.b;
    double res = 0.0, loss = 0.0;
    if (bad_row) {
      flag |= kMlrFlagBadInput;
    } else {
      bool clamped;
      loss = svc_row_terms(m, y, w, res, clamped);
      if (clamped) flag |= kMlrFlagClamped;
      sums[1] += (uint64_t)nb_quant(w * loss, a.kl);
    }
    if (a.margin) a.margin[r] = m;
    if (a.r) a.r[r] = res;
    if (a.loss_row) a.loss_row[r] = loss;
    if (res == 0.0) continue;                    // inside the margin, weight 0 or bad input
    sums[0] += (uint64_t)nb_quant(res, a.k);
    sums[2] += 1;
    for (int64_t j = s; j < e; ++j) G[a.idx[j]] += (uint64_t)nb_quant((double)a.val[j] * res, a.k);
  }
  return flag;
}

}  // namespace

template <class V>
void svc_eval_cpu(const SvcArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  const int64_t width = a.F;
  int T = threads <= 0 ? HostPool::get().size() : threads;
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, a.rows / 256));
  // thread 0 adds into the outputs themselves
  std::vector<std::vector<uint64_t>> priv(T > 1 ? T - 1 : 0);
  std::atomic<int64_t> flags{0};
  uint64_t sums0[3] = {0, 0, 0};
  const int64_t per = (a.rows + T - 1) / T;
  parallel_for(T, T, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      uint64_t *G, *sums;
      if (t == 0) {
        G = reinterpret_cast<uint64_t*>(a.Gq);
        sums = sums0;
      } else {
        priv[t - 1].assign((size_t)width + 3, 0);
        G = priv[t - 1].data();
        sums = G + width;
      }
      const int64_t f = svc_rows<V>(a, std::min(a.rows, t * per), std::min(a.rows, (t + 1) * per), G, sums);
      if (f) flags.fetch_or(f, std::memory_order_relaxed);
    }
  });
  uint64_t* out = reinterpret_cast<uint64_t*>(a.Gq);
  if (T > 1)
    parallel_for(width, threads, 1 << 14, [&](int64_t lo, int64_t hi) {
      for (const auto& p : priv)
        for (int64_t i = lo; i < hi; ++i) out[i] += p[i];
    });
  for (const auto& p : priv)
    for (int i = 0; i < 3; ++i) sums0[i] += p[width + i];
  *reinterpret_cast<uint64_t*>(a.gbq) += sums0[0];
  *reinterpret_cast<uint64_t*>(a.lossq) += sums0[1];
  *reinterpret_cast<uint64_t*>(a.nact) += sums0[2];
  *a.flag |= flags.load();
}
template void svc_eval_cpu<float>(const SvcArgs<float>&, int);
template void svc_eval_cpu<double>(const SvcArgs<double>&, int);

}  // namespace fdx
