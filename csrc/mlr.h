// Multinomial logistic regression over a CSR: the descriptor and the term functions shared by
// mlr_kernels.hip and mlr_cpu.cpp, so both sides execute the same operations (fp contraction is off
// in both). One op, mlr_eval: one function evaluation of the softmax objective on a row shard.
//   margins    m[i, c] = b_c + sum_j val[j] XS[idx[j], c] in nb_score's order (lane-strided partials
//              of 64 lanes, the xor butterfly, then + b_c), XS stored feature-major [F][C]
//   row terms  mlr_row_terms below: loss_i and the residuals r[i, c] = w_i (p_ic - [c == y_i])
//   sums       Gq[f, c] = sum rint(x_ij r_ic 2^k) over the stored entries (idx = f), feature-major,
//              gbq[c] = sum_i rint(r_ic 2^k), lossq = sum_i rint(w_i min(loss_i, 2048) 2^kl); all int64
// The sums are integers, so for given residuals they do not depend on the order of the adds: not on
// the grid, the rows per workgroup, the hot set, the host threads or the world size. The flag word
// holds two 32-bit halves, each written with ordinary stores of the value 1: the low half says that
// a row's loss was not < 2048 (such a row counts 2048), the high half names bad input (a label that
// is no integer in 0 .. C - 1, a weight that is negative or not finite, a value that is not finite,
// a feature id outside 0 .. F - 1); a row with bad input adds nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "nb.h"

#pragma clang fp contract(off)

namespace fdx {

FDX_HD bool mlr_weight_ok(double w) { return w >= 0.0 && w <= 1.79769313486231570815e308; }
FDX_HD bool mlr_value_ok(double x) { return x >= -1.79769313486231570815e308 && x <= 1.79769313486231570815e308; }

// Loss and residuals of one row from its C margins, label y (0 .. C - 1) and weight w. Returns the
// loss clamped to kMlrLossCap and sets `clamped` when it was not below it (NaN included). A margin
// that is not finite gives residuals that are not finite; they are replaced by 0, so every
// residual can be quantised (such a row is clamped, and the trainer rejects a clamped evaluation).
template <int C>
FDX_HD double mlr_row_terms(const double (&m)[C], int y, double w, double (&r)[C], bool& clamped) {
  double mx = m[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = m[c] > mx ? m[c] : mx;
  double e[C];
  double S = 0.0, my = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = exp(m[c] - mx);
    S += e[c];
    my = c == y ? m[c] : my;
  }
  const double loss = (mx - my) + log(S);
  clamped = !(loss < kMlrLossCap);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double t = w * (e[c] / S - (c == y ? 1.0 : 0.0));
    r[c] = fabs(t) <= w ? t : 0.0;
  }
  return clamped ? kMlrLossCap : loss;
}

// ---------------------------------------------------------------- descriptor
// comes first in MlrArgs: the kernel reads the coefficients with the CSR's pointers in one
// argument load, which keeps its scalar registers where they were before the parts were shared
struct MlrCoef {
  const double* XS;          // [F, num_classes] scaled coefficients, feature-major
  const double* b;           // [num_classes]
};

template <class V>
struct MlrArgs : MlrCoef, CsrRows<V>, HotSet {
  int num_classes;           // 2 .. kNbMaxClasses
  int k, kl;                 // scale exponents of the gradient terms and of the loss
  // sums, zeroed by the caller
  int64_t* Gq;               // [F, num_classes]
  int64_t* gbq;              // [num_classes]
  int64_t* lossq;            // [1]
  int64_t* flag;             // [1] kMlrFlagClamped | kMlrFlagBadInput
  // per-row outputs, each may be nullptr
  double* margin;            // [rows, num_classes]
  double* R;                 // [rows, num_classes]
  double* loss_row;          // [rows] clamped to kMlrLossCap
};

template <class V> void launch_mlr_eval(const MlrArgs<V>& a, hipStream_t stream);
template <class V> void mlr_eval_cpu(const MlrArgs<V>& a, int threads);

}  // namespace fdx
