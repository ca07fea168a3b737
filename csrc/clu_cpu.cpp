// Host twins of the bisecting KMeans and silhouette kernels (contracts in clu.h): their row bodies on
// the host pass of fixedpoint.h (private blocks, merged: the thread count does not change a bit). The
// squared norm and the dots are summed in spmv's order (64 lane-strided partials, halving adds);
// sil_score walks a tile of kKmTile means at a time as on the device.
#include <vector>

#include "clu.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

// rows [lo, hi) into the block S | Wq | cnt | costq; returns the flag
template <class V>
int64_t group_rows(const KmGroupArgs<V>& a, int64_t lo, int64_t hi, uint64_t* S, uint64_t* sums) {
  const int K = a.K, Kp = a.Kp, M = a.measure, W = a.W;
  uint64_t *Wq = sums, *cnt = sums + K, *costq = sums + 2 * K;
  int64_t flag = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const int g = a.group[r];
    if (g < 0 || g >= a.G) {
      if (g >= 0) flag = 1;
      if (a.assign) a.assign[r] = -1;
      if (a.dist) a.dist[r] = 0.0;
      continue;
    }
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !nb_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    const int c0 = W * g;
    double xp[kNbWave] = {}, p[kCluMaxWidth][kNbWave] = {};
    for (int64_t j = s; j < e; ++j) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      const double* ct = a.CT + (int64_t)f * Kp + c0;
      const int l = (int)((j - s) & (kNbWave - 1));
      bad_row |= !km_value_ok(x);
      xp[l] += x * x;
      for (int i = 0; i < W; ++i) p[i][l] += x * ct[i];
    }
    const double xn = nb_butterfly_host(xp);
    if (bad_row || !km_norm_ok(xn, M)) {
      flag = 1;
      if (a.assign) a.assign[r] = -1;
      if (a.dist) a.dist[r] = 0.0;
      continue;
    }
    const double nrm = sqrt(xn);
    double d = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c0], nb_butterfly_host(p[0]));
    int c = c0;
    if (W == 2) {
      const double d1 = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c0 + 1], nb_butterfly_host(p[1]));
      if (d1 < d) { d = d1; c = c0 + 1; }
    }
    Wq[c] += (uint64_t)nb_quant(w, a.kw);
    cnt[c] += 1;
    costq[c] += (uint64_t)nb_quant(w * d, a.kc);
    if (a.assign) a.assign[r] = c;
    if (a.dist) a.dist[r] = d;
    if (!S) continue;
    const double sx = km_row_scale(M, w, nrm);
    uint64_t* row = S + (int64_t)c * a.F;
    for (int64_t j = s; j < e; ++j) row[a.idx[j]] += (uint64_t)nb_quant(sx * (double)a.val[j], a.k);
  }
  return flag;
}

// rows [lo, hi) into silq | wq; returns the flag
template <class V>
int64_t sil_rows(const SilArgs<V>& a, int64_t lo, int64_t hi, uint64_t* sums) {
  const int K = a.K, Kp = a.Kp, M = a.measure;
  int64_t flag = 0;
  for (int64_t r = lo; r < hi; ++r) {
    const double w = a.weights ? a.weights[r] : 1.0;
    const int own_c = a.label[r];
    bool bad_row = !nb_weight_ok(w) || (uint32_t)own_c >= (uint32_t)K;
    if (!bad_row) bad_row = !(a.nw[own_c] > 0.0);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double xn = 0.0, nrm = 0.0, own = 0.0, nb = 0.0;
    bool have_nb = false;
    for (int t = 0; t < Kp && !bad_row; t += kKmTile) {
      double p[kKmTile][kNbWave] = {};
      double xp[kNbWave] = {};
      for (int64_t j = s; j < e; ++j) {
        const int32_t f = a.idx[j];
        if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
        const double x = (double)a.val[j];
        const double* mt = a.MT + (int64_t)f * Kp + t;
        const int l = (int)((j - s) & (kNbWave - 1));
        if (t == 0) {
          bad_row |= !km_value_ok(x);
          xp[l] += x * x;
        }
        for (int i = 0; i < kKmTile; ++i) p[i][l] += x * mt[i];
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
          const double d = clu_sil_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.psi[c], dot);
          if (c == own_c) own = d;
          else if (a.nw[c] > 0.0 && (!have_nb || d < nb)) { nb = d; have_nb = true; }
        }
      }
    }
    double sc = 0.0;
    if (!bad_row) {
      bool ok;
      sc = clu_silhouette(a.cnt[own_c], own, nb, a.nw[own_c], w, &ok);
      bad_row = !have_nb || !ok;
    }
    if (bad_row) {
      flag = 1;
      if (a.s) a.s[r] = 0.0;
      continue;
    }
    sums[0] += (uint64_t)nb_quant(w * sc, a.ks);
    sums[1] += (uint64_t)nb_quant(w, a.kw);
    if (a.s) a.s[r] = sc;
  }
  return flag;
}

}  // namespace

template <class V>
void km_group_step_cpu(const KmGroupArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  if ((a.W != 1 && a.W != 2) || a.G < 1 || a.W * a.G > kKmMaxK || a.K != clu_centers(a.W, a.G) ||
      a.Kp != km_padded(a.K))
    throw std::runtime_error("fdx km_group_step: W, G, K or Kp out of range");
  if (a.measure != kKmEuclidean && a.measure != kKmCosine)
    throw std::runtime_error("fdx km_group_step: unknown measure");
  const int K = a.K;
  uint64_t tail[3 * kKmMaxK] = {};                 // Wq [K] | cnt [K] | costq [K]
  const int64_t width = a.S ? (int64_t)K * a.F : 0;
  if (fx_host_pass(a.rows, threads, reinterpret_cast<uint64_t*>(a.S), width, tail, 3 * K,
                   [&](int64_t lo, int64_t hi, uint64_t* S, uint64_t* sums) {
                     return group_rows<V>(a, lo, hi, a.S ? S : nullptr, sums);
                   }))
    *a.flag = 1;
  for (int c = 0; c < K; ++c) {
    reinterpret_cast<uint64_t*>(a.Wq)[c] += tail[c];
    reinterpret_cast<uint64_t*>(a.cnt)[c] += tail[K + c];
    reinterpret_cast<uint64_t*>(a.costq)[c] += tail[2 * K + c];
  }
}
template void km_group_step_cpu<float>(const KmGroupArgs<float>&, int);
template void km_group_step_cpu<double>(const KmGroupArgs<double>&, int);

template <class V>
void sil_score_cpu(const SilArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  if (a.K < 2 || a.K > kKmMaxK || a.Kp != km_padded(a.K)) throw std::runtime_error("fdx sil_score: K out of range");
  if (a.measure != kKmEuclidean && a.measure != kKmCosine) throw std::runtime_error("fdx sil_score: unknown measure");
  uint64_t tail[2] = {};
  if (fx_host_pass(a.rows, threads, nullptr, 0, tail, 2,
                   [&](int64_t lo, int64_t hi, uint64_t*, uint64_t* sums) { return sil_rows<V>(a, lo, hi, sums); }))
    *a.flag = 1;
  *reinterpret_cast<uint64_t*>(a.silq) += tail[0];
  *reinterpret_cast<uint64_t*>(a.wq) += tail[1];
}
template void sil_score_cpu<float>(const SilArgs<float>&, int);
template void sil_score_cpu<double>(const SilArgs<double>&, int);

}  // namespace fdx
