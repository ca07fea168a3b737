// Bisecting KMeans and the silhouette over a CSR: descriptors and the term functions shared by
// clu_kernels.hip and clu_cpu.cpp, so both sides execute the same operations (fp contraction is off
// in both). Two ops, both variants of km_step's wave-per-row pass (km.h) with other tails:
//   km_group_step  a Lloyd step in which the caller names each row's candidates: row r with
//                  g = group[r] competes among the W (1 or 2) adjacent centers W g .. W g + W - 1.
//                  g < 0 skips the row (only group[r] is read), g >= G is bad input. One walk in
//                  spmv's order gives the squared norm and the W dots (W = 2: one 16-byte read of
//                  CT per entry), then d_i = km_distance(...), a = (W == 2 && d_1 < d_0) ? 1 : 0
//                  (the left child wins ties), c = W g + a, and the exact int64 sums into cluster c:
//                  S[c, f] += rint(s x 2^k), Wq[c] += rint(w 2^kw), cnt[c] += 1 and the per-cluster
//                  costq[c] += rint(w d_a 2^kc). Without S (assign-only) the second walk is skipped.
//   sil_score      Spark's silhouette coefficient of every row from per-cluster statistics (the
//                  means MT [F][Kp], psi, the weight sums nw and the row counts cnt): the dots and
//                  the squared norm from km_step's tile loop, D_c = (xn + psi_c) - 2 dot_c
//                  (unclamped, Spark's formula) or 1 - dot_c / sqrt(xn), own = D_a of the row's label
//                  a, nb the least D_c over the other present clusters (ascending, strict <), the
//                  coefficient by clu_silhouette, and the exact sums silq += rint(w s 2^ks),
//                  wq += rint(w 2^kw).
// Neither op uses exp or log; sqrt and the division are correctly rounded on both sides. The sums
// are integers, so a block is a function of its inputs alone: not of the grid, the rows per
// workgroup, the hot set, the host threads or the world size. Bad input sets a flag word; such a row
// adds nothing, and the caller raises.
#pragma once
#include "km.h"

#pragma clang fp contract(off)

namespace fdx {

constexpr int kCluMaxWidth = 2;                    // candidates of a row in km_group_step
static_assert(kKmMaxTableBytes + 3 * kKmMaxK * 8 <= 64 * 1024, "table and the three [64] sums fit 64 KiB");
static_assert(kKmTile % kCluMaxWidth == 0, "a pair of children is 16-byte aligned in a row of CT");

// centers of a km_group_step pass of G groups of W candidates
constexpr int clu_centers(int W, int G) { return W * G < 2 ? 2 : W * G; }

// what a row's distance to cluster c is in the silhouette (psi_c = 0 under cosine)
FDX_HD double clu_sil_distance(int measure, double xn, double nrm, double psi_c, double dot_c) {
  if (measure == kKmCosine) return 1.0 - dot_c / nrm;
  return (xn + psi_c) - 2.0 * dot_c;
}

// The silhouette coefficient of a row of weight w in a cluster of cnt_a rows and the weight sum
// nw_a: own_raw its distance to its own cluster, nb the least distance to another one. *ok is false
// for nw_a - w not > 0 (non-singleton) or a result that is not finite.
FDX_HD double clu_silhouette(int cnt_a, double own_raw, double nb, double nw_a, double w, bool* ok) {
  *ok = true;
  if (cnt_a == 1) return 0.0;
  const double rest = nw_a - w;
  if (!(rest > 0.0)) { *ok = false; return 0.0; }
  const double own = (own_raw * nw_a) / rest;
  const double s = own < nb ? 1.0 - own / nb : own > nb ? nb / own - 1.0 : 0.0;
  *ok = km_value_ok(own) && km_value_ok(nb) && km_value_ok(s);
  return *ok ? s : 0.0;
}

// ---------------------------------------------------------------- descriptors
template <class V>
struct KmGroupArgs : CsrRows<V>, HotSet {          // the labels are unused
  int W;                     // 1 or 2
  int G;                     // groups, W G <= kKmMaxK
  int K;                     // clu_centers(W, G)
  int Kp;                    // km_padded(K)
  int measure;
  int k, kw, kc;
  const int32_t* group;      // [rows] < 0: skipped; >= G: bad input
  const double* CT;          // [F, Kp], 16-byte aligned
  const double* cn;          // [Kp]
  // outputs, zeroed by the caller
  int64_t* S;                // [K, F], or nullptr: assign only
  int64_t* Wq;               // [K]
  int64_t* cnt;              // [K]
  int64_t* costq;            // [K]
  int64_t* flag;             // [1]
  // per-row outputs, or nullptr
  int32_t* assign;           // [rows] cluster of the row, -1 for a skipped or a flagged row
  double* dist;              // [rows] distance to it, 0 for those
};

template <class V>
struct SilArgs : CsrRows<V>, HotSet {              // the double labels and the hot set are unused
  int K, Kp;
  int measure;
  int ks, kw;
  const int32_t* label;      // [rows]
  const double* MT;          // [F, Kp] cluster means, feature-major, padding columns zero
  const double* psi;         // [Kp]
  const double* nw;          // [Kp] weight sums, 0.0 for an absent cluster
  const int32_t* cnt;        // [Kp] rows of a cluster
  // outputs, zeroed by the caller
  int64_t* silq;             // [1]
  int64_t* wq;               // [1]
  int64_t* flag;             // [1]
  double* s;                 // [rows] or nullptr: the coefficient of a row, 0 for a flagged row
};

template <class V> void launch_km_group_step(const KmGroupArgs<V>& a, hipStream_t stream);
template <class V> void km_group_step_cpu(const KmGroupArgs<V>& a, int threads);
template <class V> void launch_sil_score(const SilArgs<V>& a, hipStream_t stream);
template <class V> void sil_score_cpu(const SilArgs<V>& a, int threads);

}  // namespace fdx
