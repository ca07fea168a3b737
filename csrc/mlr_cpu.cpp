// Host twin of the multinomial logistic regression kernel (contract in mlr.h): its row body on the
// host pass of fixedpoint.h (private blocks, merged: the thread count does not change a bit).
// Margins are summed in nb_score's order (64 lane-strided partials, halving adds, then + b_c); the
// row terms are mlr_row_terms, as on the device.
#include <stdexcept>

#include "mlr.h"

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
  uint64_t tail[C + 1] = {};                       // gbq [C] | lossq
  *a.flag |= fx_host_pass(a.rows, threads, reinterpret_cast<uint64_t*>(a.Gq), (int64_t)C * a.F, tail, C + 1,
                          [&](int64_t lo, int64_t hi, uint64_t* G, uint64_t* sums) {
                            return mlr_rows<V, C>(a, lo, hi, G, sums, sums + C);
                          });
  for (int c = 0; c < C; ++c) reinterpret_cast<uint64_t*>(a.gbq)[c] += tail[c];
  *reinterpret_cast<uint64_t*>(a.lossq) += tail[C];
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
