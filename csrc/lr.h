// Elastic-net logistic regression (OWL-QN): descriptors and the per-row / per-element terms shared
// by lr_kernels.hip and lr_cpu.cpp, so both sides execute the same operations (fp contraction is
// off in both). Four ops:
//   lr_forward      margin, residual r = w (sigma(m) - y) and log-loss of every row of a CSR, plus
//                   one (sum w loss, sum r) partial per kLrRowsPerPartial rows
//   lr_reduce       K rows of partials -> K sums in one fixed order
//   lr_owlqn_step   x_new = pi(x + t d; xi), xs_new = scale x_new[:F], partials of |x_new|_1,
//                   x_new . x_new and pg . (x_new - x)
//   lr_pseudo_grad  smooth gradient, pseudo-gradient and orthant of the L1 term, partials of |pg|^2
// The parameter vector has F + 1 slots: F coefficients and the intercept (never penalised, never
// projected). No kernel uses an atomic: every sum has one order that depends on sizes alone.
#pragma once
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace fdx {

constexpr int kLrWave = 64;
constexpr int kLrBlock = 256;                           // lanes of every workgroup of the four kernels
constexpr int kLrRowsPerPartial = kLrBlock / kLrWave;   // lr_forward: one wave per row, one partial per workgroup
constexpr int kLrReduceBlock = 256;                     // lr_reduce: strided partial sums, then a tree of this width
constexpr int kLrMaxGroups = 1024;                      // workgroups of a parameter pass (grid-stride beyond)

// ---------------------------------------------------------------- per-row terms
struct LrRowTerms {
  double loss, r;
};

// loss = log(1 + e^m) - y m (stable form), r = w (sigma(m) - y); sigma never overflows: e <= 1.
FDX_HD LrRowTerms lr_row_terms(double m, double y, double w) {
  const double e = exp(-fabs(m));
  const double d = 1.0 + e;
  const double s = m >= 0.0 ? 1.0 / d : e / d;
  LrRowTerms t;
  t.loss = (m > 0.0 ? m : 0.0) - m * y + log1p(e);
  t.r = w * (s - y);
  return t;
}

// ---------------------------------------------------------------- per-parameter terms
struct LrStepTerms {
  double x_new, xs_new, l1, sq, dec;
};

// pi(x + t d; xi): a coefficient that leaves its orthant becomes exactly +0.0
FDX_HD LrStepTerms lr_step_terms(double x, double d, double xi, double pg, double scale, double t, bool coef) {
  const double v = x + t * d;
  const bool keep = !coef || (xi > 0.0 && v > 0.0) || (xi < 0.0 && v < 0.0);
  LrStepTerms o;
  o.x_new = keep ? v : 0.0;
  o.xs_new = scale * o.x_new;
  o.l1 = coef ? fabs(o.x_new) : 0.0;
  o.sq = coef ? o.x_new * o.x_new : 0.0;
  o.dec = pg * (o.x_new - x);
  return o;
}

struct LrGradTerms {
  double g, pg, xi;
};

// coefficient j < F: g = scale xtr / W + l2 beta; pseudo-gradient and orthant of l1 |beta|
FDX_HD LrGradTerms lr_grad_terms(double xtr, double scale, double W, double beta, double l1, double l2) {
  LrGradTerms o;
  o.g = scale * xtr / W + l2 * beta;
  const double up = o.g + l1, dn = o.g - l1;
  if (beta > 0.0) o.pg = up;
  else if (beta < 0.0) o.pg = dn;
  else o.pg = up < 0.0 ? up : (dn > 0.0 ? dn : 0.0);
  if (beta > 0.0) o.xi = 1.0;
  else if (beta < 0.0) o.xi = -1.0;
  else o.xi = o.pg < 0.0 ? 1.0 : (o.pg > 0.0 ? -1.0 : 0.0);
  return o;
}

// ---------------------------------------------------------------- layout of the sums
inline int64_t lr_forward_partials(int64_t rows) { return (rows + kLrRowsPerPartial - 1) / kLrRowsPerPartial; }

// workgroups of a pass over n parameters: every lane takes pairs (2p, 2p + 1), p = lane id, + grid size, ...
inline int64_t lr_param_groups(int64_t n) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t g = (pairs + kLrBlock - 1) / kLrBlock;
  return g < 1 ? 1 : (g > kLrMaxGroups ? kLrMaxGroups : g);
}

template <class V>
struct LrForwardArgs {
  const int64_t* indptr;   // [rows + 1]
  const int32_t* idx;
  const V* val;
  int64_t rows;
  const double* xs;        // [F] scale * beta
  const double* b;         // [1] intercept (0 when none is fitted)
  const double* y;         // [rows] labels in {0, 1}
  const double* w;         // [rows]
  double* r;               // [rows]
  double* loss_row;        // [rows] or null
  double* margin;          // [rows] or null
  double* partials;        // [2, lr_forward_partials(rows)]: sum w loss, sum r
};

struct LrReduceArgs {
  const double* partials;  // [K, P]
  int64_t K, P;
  double* out;             // [K]
};

struct LrStepArgs {
  const double* x;         // [n] n = F + 1
  const double* d;         // [n]
  const double* xi;        // [n]
  const double* pg;        // [n]
  const double* scale;     // [F]
  double t;
  int64_t F;
  double* x_new;           // [n]
  double* xs_new;          // [F]
  double* partials;        // [3, lr_param_groups(n)]: l1, sq, dec
};

struct LrGradArgs {
  const double* parts;     // [F + 2]: sum w loss, sum r, X^T r (summed over ranks)
  const double* scale;     // [F]
  const double* x;         // [F + 1]
  double W, l1, l2;
  int64_t F;
  bool fit_intercept;
  double* g;               // [F + 1]
  double* pg;              // [F + 1]
  double* xi;              // [F + 1]
  double* partials;        // [lr_param_groups(F + 1)]: pg . pg
};

// Tree of fixed shape over kLrReduceBlock slots (the host twin runs the same loop).
inline double lr_tree_host(double* s) {
  for (int o = kLrReduceBlock / 2; o > 0; o >>= 1)
    for (int t = 0; t < o; ++t) s[t] += s[t + o];
  return s[0];
}

}  // namespace fdx
