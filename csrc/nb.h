// Naive Bayes over a CSR: descriptors and the term functions shared by nb_kernels.hip and
// nb_cpu.cpp, so both sides execute the same operations (fp contraction is off in both). Two ops:
//   nb_sums    S[c, f] = sum of q = rint(w_i x_ij 2^k) over the stored entries (idx = f) of the rows
//              with label c, Wq[c] = sum of rint(w_i 2^kw), cnt[c] = rows of class c; all int64
//   nb_score   raw[r, c] = b_c + sum_j val[j] W[idx[j], c] in spmv's order (lane-strided partials
//              of 64 lanes, the xor butterfly, then + b_c), W stored feature-major [F][C]
// The sums are integers, so they do not depend on the order of the adds: not on the grid, the rows
// per workgroup, the hot set, the host threads or the world size. Bad input (a label that is no
// integer in 0 .. C - 1, a weight that is not finite and > 0, a value that is negative, not finite
// or, for Bernoulli, neither 0 nor 1, a feature id outside 0 .. F - 1) sets a flag word; such rows
// and entries add nothing, and the caller raises before any model is produced.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "fixedpoint.h"

#pragma clang fp contract(off)

namespace fdx {

// q = rint(t 2^k) as int64, ties to even; the scaling by a power of two is exact
FDX_HD int64_t nb_quant(double t, int k) { return (int64_t)rint(ldexp(t, k)); }

// class of a label, or -1: an integer in 0 .. num_classes - 1
FDX_HD int nb_label(double y, int num_classes) {
  if (!(y >= 0.0) || !(y < (double)num_classes)) return -1;
  const int c = (int)y;
  return (double)c == y ? c : -1;
}

FDX_HD bool nb_weight_ok(double w) { return w > 0.0 && w <= 1.79769313486231570815e308; }

// a stored value a model may be fitted on
FDX_HD bool nb_value_ok(double x, bool bernoulli) {
  return bernoulli ? (x == 0.0 || x == 1.0) : (x >= 0.0 && x <= 1.79769313486231570815e308);
}

// ---------------------------------------------------------------- descriptors
template <class V>
struct NbSumArgs : CsrRows<V>, HotSet {
  int num_classes;           // 2 .. kNbMaxClasses
  int k, kw;                 // scale exponents of the terms and of the weights
  bool bernoulli;
  // outputs, zeroed by the caller
  int64_t* S;                // [num_classes, F]
  int64_t* Wq;               // [num_classes]
  int64_t* cnt;              // [num_classes]
  int64_t* flag;             // [1] set to 1 on bad input
};

template <class V>
struct NbScoreArgs {
  const int64_t* indptr;     // [rows + 1]
  const int32_t* idx;
  const V* val;
  int64_t rows;
  int32_t F;
  int num_classes;           // 2 .. kNbMaxClasses
  const double* W;           // [F, num_classes]
  const double* b;           // [num_classes]
  double* out;               // [rows, num_classes]
};

template <class V> void launch_nb_sums(const NbSumArgs<V>& a, hipStream_t stream);
template <class V> void nb_sums_cpu(const NbSumArgs<V>& a, int threads);
template <class V> void launch_nb_score(const NbScoreArgs<V>& a, hipStream_t stream);
template <class V> void nb_score_cpu(const NbScoreArgs<V>& a, int threads);

}  // namespace fdx
