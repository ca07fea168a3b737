// Host twin of the linear SVC kernel (contract in svc.h): its row body on the host pass of
// fixedpoint.h (private blocks, merged: the thread count does not change a bit). The margin is
// summed in spmv's order (64 lane-strided partials, halving adds, then + b); the row terms are
// svc_row_terms, as on the device, so the block equals the device's.
#include "svc.h"

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
  uint64_t tail[3] = {};                           // gbq, lossq, nact
  *a.flag |= fx_host_pass(a.rows, threads, reinterpret_cast<uint64_t*>(a.Gq), a.F, tail, 3,
                          [&](int64_t lo, int64_t hi, uint64_t* G, uint64_t* sums) {
                            return svc_rows<V>(a, lo, hi, G, sums);
                          });
  *reinterpret_cast<uint64_t*>(a.gbq) += tail[0];
  *reinterpret_cast<uint64_t*>(a.lossq) += tail[1];
  *reinterpret_cast<uint64_t*>(a.nact) += tail[2];
}
template void svc_eval_cpu<float>(const SvcArgs<float>&, int);
template void svc_eval_cpu<double>(const SvcArgs<double>&, int);

}  // namespace fdx
