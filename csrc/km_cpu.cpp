// Host twins of the KMeans kernels (contracts in km.h). km_step is its row body on the host pass of
// fixedpoint.h (private blocks, merged: the thread count does not change a bit); the squared norm
// and the dots are summed in spmv's order (64 lane-strided partials, halving adds), a tile of
// kKmTile centers at a time as on the device. km_centers sums over the features in the device's
// order: kKmCentersBlock strided partials, then the tree of km_tree_host.
#include <vector>

#include "km.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

// rows [lo, hi) into the block S | Wq | cnt | costq; returns the flag
template <class V>
int64_t km_rows(const KmStepArgs<V>& a, int64_t lo, int64_t hi, uint64_t* S, uint64_t* sums) {
  const int K = a.K, Kp = a.Kp, M = a.measure;
  uint64_t *Wq = sums, *cnt = sums + K, *costq = sums + 2 * K;
  int64_t flag = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !nb_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double xn = 0.0, nrm = 0.0, best_d = 0.0;
    int best_c = 0;
    for (int t = 0; t < Kp; t += kKmTile) {
      double p[kKmTile][kNbWave] = {};
      double xp[kNbWave] = {};
      for (int64_t j = s; j < e; ++j) {
        const int32_t f = a.idx[j];
        if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
        const double x = (double)a.val[j];
        const double* ct = a.CT + (int64_t)f * Kp + t;
        const int l = (int)((j - s) & (kNbWave - 1));
        if (t == 0) {
          bad_row |= !km_value_ok(x);
          xp[l] += x * x;
        }
        for (int i = 0; i < kKmTile; ++i) p[i][l] += x * ct[i];
      }
      if (t == 0) {
        xn = nb_butterfly_host(xp);
        bad_row = bad_row || !km_norm_ok(xn, M);
        if (bad_row) break;
        nrm = sqrt(xn);
      }
      for (int i = 0; i < kKmTile; ++i) {
        const double dot = nb_butterfly_host(p[i]);
        const int c = t + i;
        if (c < K) {
          const double d = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c], dot);
          if (c == 0 || d < best_d) { best_d = d; best_c = c; }
        }
      }
    }
    if (bad_row) {
      flag = 1;
      if (a.assign) a.assign[r] = -1;
      if (a.dist) a.dist[r] = 0.0;
      continue;
    }
    const int c = best_c;
    Wq[c] += (uint64_t)nb_quant(w, a.kw);
    cnt[c] += 1;
    *costq += (uint64_t)nb_quant(w * best_d, a.kc);
    if (a.assign) a.assign[r] = c;
    if (a.dist) a.dist[r] = best_d;
    if (!S) continue;
    const double sx = km_row_scale(M, w, nrm);
    uint64_t* row = S + (int64_t)c * a.F;
    for (int64_t j = s; j < e; ++j) row[a.idx[j]] += (uint64_t)nb_quant(sx * (double)a.val[j], a.k);
  }
  return flag;
}

}  // namespace

template <class V>
void km_step_cpu(const KmStepArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  if (a.K < 2 || a.K > kKmMaxK || a.Kp != km_padded(a.K)) throw std::runtime_error("fdx km_step: K out of range");
  if (a.measure != kKmEuclidean && a.measure != kKmCosine) throw std::runtime_error("fdx km_step: unknown measure");
  const int K = a.K;
  uint64_t tail[2 * kKmMaxK + 1] = {};             // Wq [K] | cnt [K] | costq
  const int64_t width = a.S ? (int64_t)K * a.F : 0;
  if (fx_host_pass(a.rows, threads, reinterpret_cast<uint64_t*>(a.S), width, tail, 2 * K + 1,
                   [&](int64_t lo, int64_t hi, uint64_t* S, uint64_t* sums) {
                     return km_rows<V>(a, lo, hi, a.S ? S : nullptr, sums);
                   }))
    *a.flag = 1;
  for (int c = 0; c < K; ++c) {
    reinterpret_cast<uint64_t*>(a.Wq)[c] += tail[c];
    reinterpret_cast<uint64_t*>(a.cnt)[c] += tail[K + c];
  }
  *reinterpret_cast<uint64_t*>(a.costq) += tail[2 * K];
}
template void km_step_cpu<float>(const KmStepArgs<float>&, int);
template void km_step_cpu<double>(const KmStepArgs<double>&, int);

void km_centers_cpu(const KmCentersArgs& a, int threads) {
  if (a.K < 2 || a.K > kKmMaxK || a.Kp != km_padded(a.K) || a.F < 1)
    throw std::runtime_error("fdx km_centers: K or F out of range");
  const int64_t Kp = a.Kp;
  parallel_for(a.K, threads, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t c = lo; c < hi; ++c) {
      const int64_t wq = a.Wq[c];
      const bool keep = wq == 0;
      const double W = ldexp((double)wq, -a.kw);
      const int64_t* S = a.S + c * a.F;
      double s[kKmCentersBlock];
      double inv = 1.0;
      if (!keep && a.measure == kKmCosine) {
        for (int t = 0; t < kKmCentersBlock; ++t) s[t] = 0.0;
        for (int32_t f = 0; f < a.F; ++f) {        // slot f mod 256 adds its features ascending
          const double m = km_mean(S[f], a.k, W);
          s[f & (kKmCentersBlock - 1)] += m * m;
        }
        inv = sqrt(km_tree_host(s));
        if (inv == 0.0) inv = 1.0;
      }
      double nn[kKmCentersBlock] = {}, mv[kKmCentersBlock] = {};
      for (int32_t f = 0; f < a.F; ++f) {
        const double old = a.CT_old[f * Kp + c];
        double v = old;
        if (!keep) {
          v = km_mean(S[f], a.k, W);
          if (a.measure == kKmCosine) v = v / inv;
        }
        a.CT_new[f * Kp + c] = v;
        nn[f & (kKmCentersBlock - 1)] += v * v;
        const double d = v - old;
        mv[f & (kKmCentersBlock - 1)] += d * d;
      }
      a.cn_new[c] = km_tree_host(nn);
      a.moved2[c] = km_tree_host(mv);
    }
  });
}

}  // namespace fdx
