// Linear support vector classification (hinge loss) over a CSR: the descriptor and the term function
// shared by svc_kernels.hip and svc_cpu.cpp, so both sides execute the same operations (fp
// contraction is off in both). One op, svc_eval: one function evaluation of the hinge objective on
// a row shard.
//   margin     m_i = b + sum_j val[j] xs[idx[j]] in spmv's order (lane l of 64 adds the entries
//              l, l + 64, ... ascending, multiply then add, the xor butterfly over 32 .. 1, then + b),
//              so m is spmv(X, xs) + b bit for bit
//   row terms  svc_row_terms below (Spark's HingeAggregator): s = 2 y - 1, z = 1 - s m,
//              loss_i = max(z, 0) capped at 2048, r_i = z > 0 ? - s w_i : 0; a row with z == 0 is inactive
//   sums       Gq[f] = sum rint((x_ij r_i) 2^k) over the stored entries (idx = f), gbq = sum_i rint(r_i 2^k),
//              lossq = sum_i rint((w_i loss_i) 2^kl), nact = rows with r_i != 0; all int64
// Every term is exactly rounded fp64 arithmetic (no exp, no log) and the sums are integers, so the
// whole block [Gq (F) | gbq | lossq | nact | flag], lossq included, is a pure function of the inputs:
// it does not depend on the grid, the rows per workgroup, the hot set, the host thread count, the
// backend (host and device give the same bits) or the world size. The flag word is fixedpoint.h's: two
// 32-bit halves, each written with ordinary stores of the value 1; the low half says that a row's
// z was not < 2048 (NaN included; such a row's loss counts 2048), the high half names bad input (a
// label other than 0 / 1, a weight that is negative or not finite, a value that is not finite, a
// feature id outside 0 .. F - 1); a row with bad input adds nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mlr.h"

#pragma clang fp contract(off)

namespace fdx {

// Hinge terms of one row from its margin m, label y (0 or 1) and weight w: returns the loss capped
// at kMlrLossCap, sets `clamped` when z was not below it (a NaN margin included) and r to the
// row's residual (d loss / d m times w), which is 0 for a row inside the margin (z <= 0).
FDX_HD double svc_row_terms(double m, double y, double w, double& r, bool& clamped) {
  const double s = 2.0 * y - 1.0;
  const double z = 1.0 - s * m;
  clamped = !(z < kMlrLossCap);
  r = z > 0.0 ? -s * w : 0.0;
  return clamped ? kMlrLossCap : (z > 0.0 ? z : 0.0);
}

FDX_HD bool svc_label_ok(double y) { return y == 0.0 || y == 1.0; }

// ---------------------------------------------------------------- descriptor
template <class V>
struct SvcArgs : CsrRows<V>, HotSet {   // labels are 0 or 1
  const double* xs;          // [F] scaled coefficients
  double b;                  // intercept
  int k, kl;                 // scale exponents of the gradient terms and of the loss
  // sums, zeroed by the caller
  int64_t* Gq;               // [F]
  int64_t* gbq;              // [1]
  int64_t* lossq;            // [1]
  int64_t* nact;             // [1] rows with a non-zero residual
  int64_t* flag;             // [1] kMlrFlagClamped | kMlrFlagBadInput
  // per-row outputs, each may be nullptr
  double* margin;            // [rows]
  double* r;                 // [rows]
  double* loss_row;          // [rows] capped at kMlrLossCap
};

template <class V> void launch_svc_eval(const SvcArgs<V>& a, hipStream_t stream);
template <class V> void svc_eval_cpu(const SvcArgs<V>& a, int threads);

}  // namespace fdx
