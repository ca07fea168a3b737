// KMeans over a CSR: descriptors and the term functions shared by km_kernels.hip and km_cpu.cpp, so
// both sides execute the same operations (fp contraction is off in both). Two ops:
//   km_step     one Lloyd evaluation over a row shard: every row's distances to the K centers (dot
//               products against the feature-major centers CT [F][Kp] in spmv's order: lane-strided
//               partials of 64 lanes, the xor butterfly), its cluster a (the smallest c that attains
//               the least distance), and the exact int64 sums of the fixed-point row pass
//               (fixedpoint.h) into cluster a: S[a, f] += rint(s x 2^k), Wq[a] += rint(w 2^kw),
//               cnt[a] += 1, costq += rint(w d_a 2^kc). Without S (assign-only) the second walk is
//               skipped: prediction, the cost of a model and the seeding.
//   km_centers  the update from the summed S and Wq: mean_f = S[c, f] 2^-k / (Wq[c] 2^-kw), for the
//               cosine measure divided by its norm; the squared norms of the new centers and the
//               squared distance each centre moved. Every sum over the features has a fixed order:
//               lane t of 256 adds features t, t + 256, ... ascending, then the tree of lr_tree_host.
// The sums are integers, so they do not depend on the order of the adds: not on the grid, the rows
// per workgroup, the hot set, the host threads or the world size. Bad input (a feature id outside
// 0 .. F - 1, a value that is not finite, a row whose squared norm is not finite, a weight that is
// not finite and > 0, a zero row under the cosine measure) sets a flag word; such a row adds
// nothing and is assigned -1, and the caller raises before any model is produced.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "fixedpoint.h"
#include "nb.h"

#pragma clang fp contract(off)

namespace fdx {

constexpr int kKmMaxK = 64;                        // most centers of a pass (a lane of the wave per cluster)
constexpr int kKmTile = 8;                         // centers whose partial dots a lane holds in registers
constexpr int kKmMaxTableBytes = 62 * 1024;        // with the 2 K + 1 scalar sums a workgroup stays within 64 KiB
constexpr int kKmCentersBlock = 256;               // km_centers: strided partial sums, then a tree of this width
enum : int { kKmEuclidean = 0, kKmCosine = 1 };

static_assert(kKmMaxK <= kNbWave, "a lane of the wave keeps the sums of one cluster");
static_assert(kKmMaxTableBytes + (2 * kKmMaxK + 1) * 8 <= 64 * 1024, "table and scalar sums fit 64 KiB");

constexpr int km_padded(int K) { return (K + kKmTile - 1) / kKmTile * kKmTile; }

FDX_HD bool km_value_ok(double x) { return x >= -1.79769313486231570815e308 && x <= 1.79769313486231570815e308; }

// what the squared norm of a row must be: finite, and not 0 under the cosine measure
FDX_HD bool km_norm_ok(double xn, int measure) {
  return xn <= 1.79769313486231570815e308 && (measure != kKmCosine || xn > 0.0);
}

// distance of a row (squared norm xn, nrm = sqrt(xn)) to a center (squared norm cn_c, dot product dot_c)
FDX_HD double km_distance(int measure, double xn, double nrm, double cn_c, double dot_c) {
  if (measure == kKmCosine) return 1.0 - dot_c / nrm;
  return fmax((xn + cn_c) - 2.0 * dot_c, 0.0);
}

// the factor of a row's entries in the sums of its cluster
FDX_HD double km_row_scale(int measure, double w, double nrm) { return measure == kKmCosine ? w / nrm : w; }

// feature f of the mean of a cluster with the weight sum W
FDX_HD double km_mean(int64_t s, int k, double W) { return ldexp((double)s, -k) / W; }

// ---------------------------------------------------------------- descriptors
template <class V>
struct KmStepArgs : CsrRows<V>, HotSet {           // the labels are unused
  int K;                     // 2 .. kKmMaxK
  int Kp;                    // km_padded(K)
  int measure;               // kKmEuclidean / kKmCosine
  int k, kw, kc;             // scale exponents of the coordinates, the weights and the cost
  const double* CT;          // [F, Kp] centers, feature-major, padding columns zero
  const double* cn;          // [Kp] squared norms of the centers (euclidean)
  // outputs, zeroed by the caller
  int64_t* S;                // [K, F], or nullptr: assign only
  int64_t* Wq;               // [K]
  int64_t* cnt;              // [K]
  int64_t* costq;            // [1]
  int64_t* flag;             // [1] set to 1 on bad input
  // per-row outputs, or nullptr
  int32_t* assign;           // [rows] cluster of the row, -1 for a flagged row
  double* dist;              // [rows] distance to it
};

struct KmCentersArgs {
  int K, Kp;
  int32_t F;
  int measure;
  int k, kw;
  const int64_t* S;          // [K, F]
  const int64_t* Wq;         // [K]
  const double* CT_old;      // [F, Kp]
  double* CT_new;            // [F, Kp], padding columns left as they are (the caller zeroes them)
  double* cn_new;            // [Kp] entries 0 .. K - 1 written
  double* moved2;            // [K]
};

template <class V> void launch_km_step(const KmStepArgs<V>& a, hipStream_t stream);
template <class V> void km_step_cpu(const KmStepArgs<V>& a, int threads);
void launch_km_centers(const KmCentersArgs& a, hipStream_t stream);
void km_centers_cpu(const KmCentersArgs& a, int threads);

// Tree of fixed shape over kKmCentersBlock slots (lr_tree_host's shape; the device runs the same loop).
inline double km_tree_host(double* s) {
  for (int o = kKmCentersBlock / 2; o > 0; o >>= 1)
    for (int t = 0; t < o; ++t) s[t] += s[t + o];
  return s[0];
}

}  // namespace fdx
