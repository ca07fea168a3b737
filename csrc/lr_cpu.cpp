// Host twins of the elastic-net logistic-regression kernels (same contracts and partial layout as
// lr_kernels.hip: one partial per kLrRowsPerPartial rows added in row order, per-lane strided sums
// in ascending order, the tree of lr_tree_host), so given equal per-row terms every sum is bitwise
// the device's.
#include <algorithm>
#include <vector>

#include "lr.h"
#include "ops.h"
#include "parallel_for.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {
inline double lr_butterfly(double* p) {
  for (int o = 32; o > 0; o >>= 1)
    for (int l = 0; l < 64; ++l)
      if (l < (l ^ o)) { const double t = p[l] + p[l ^ o]; p[l] = t; p[l ^ o] = t; }
  return p[0];
}
}  // namespace

template <class V>
void lr_forward_cpu(const LrForwardArgs<V>& a, int threads) {
  const int64_t P = lr_forward_partials(a.rows);
  parallel_for(P, threads, 256, [&](int64_t lo, int64_t hi) {
    for (int64_t blk = lo; blk < hi; ++blk) {
      double s0 = 0.0, s1 = 0.0;
      const int64_t r0 = blk * kLrRowsPerPartial;
      for (int64_t r = r0; r < r0 + kLrRowsPerPartial && r < a.rows; ++r) {
        double p[64] = {0};
        const int64_t s = a.indptr[r], e = a.indptr[r + 1];
        for (int64_t j = s; j < e; ++j) p[(j - s) & 63] += (double)a.val[j] * a.xs[a.idx[j]];
        const double m = lr_butterfly(p) + a.b[0];
        const double w = a.w[r];
        const LrRowTerms t = lr_row_terms(m, a.y[r], w);
        a.r[r] = t.r;
        if (a.loss_row) a.loss_row[r] = t.loss;
        if (a.margin) a.margin[r] = m;
        s0 += w * t.loss;
        s1 += t.r;
      }
      a.partials[blk] = s0;
      a.partials[P + blk] = s1;
    }
  });
}
template void lr_forward_cpu<float>(const LrForwardArgs<float>&, int);
template void lr_forward_cpu<double>(const LrForwardArgs<double>&, int);

void lr_reduce_cpu(const LrReduceArgs& a) {
  for (int64_t k = 0; k < a.K; ++k) {
    const double* p = a.partials + k * a.P;
    double s[kLrReduceBlock];
    for (int t = 0; t < kLrReduceBlock; ++t) {
      double acc = 0.0;
      for (int64_t i = t; i < a.P; i += kLrReduceBlock) acc += p[i];
      s[t] = acc;
    }
    a.out[k] = lr_tree_host(s);
  }
}

void lr_owlqn_step_cpu(const LrStepArgs& a, int threads) {
  const int64_t n = a.F + 1, pairs = (n + 1) / 2, G = lr_param_groups(n);
  parallel_for(G, threads, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t b = lo; b < hi; ++b) {
      double s[3][kLrBlock];
      for (int t = 0; t < kLrBlock; ++t) {
        double l1 = 0.0, sq = 0.0, dec = 0.0;
        for (int64_t p = b * kLrBlock + t; p < pairs; p += G * kLrBlock)
          for (int64_t jj = 2 * p; jj < 2 * p + 2 && jj < n; ++jj) {
            const bool coef = jj < a.F;
            const LrStepTerms u = lr_step_terms(a.x[jj], a.d[jj], a.xi[jj], a.pg[jj], coef ? a.scale[jj] : 0.0, a.t, coef);
            a.x_new[jj] = u.x_new;
            if (coef) a.xs_new[jj] = u.xs_new;
            l1 += u.l1; sq += u.sq; dec += u.dec;
          }
        s[0][t] = l1;
        s[1][t] = sq;
        s[2][t] = dec;
      }
      for (int k = 0; k < 3; ++k) a.partials[k * G + b] = lr_tree_host(s[k]);
    }
  });
}

void lr_pseudo_grad_cpu(const LrGradArgs& a, int threads) {
  const int64_t n = a.F + 1, pairs = (n + 1) / 2, G = lr_param_groups(n);
  const double* xtr = a.parts + 2;
  parallel_for(G, threads, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t b = lo; b < hi; ++b) {
      double s[kLrBlock];
      for (int t = 0; t < kLrBlock; ++t) {
        double nn = 0.0;
        for (int64_t p = b * kLrBlock + t; p < pairs; p += G * kLrBlock)
          for (int64_t jj = 2 * p; jj < 2 * p + 2 && jj < n; ++jj) {
            LrGradTerms u;
            if (jj < a.F) {
              u = lr_grad_terms(xtr[jj], a.scale[jj], a.W, a.x[jj], a.l1, a.l2);
            } else {
              u.g = a.fit_intercept ? a.parts[1] / a.W : 0.0;
              u.pg = u.g;
              u.xi = 0.0;
            }
            a.g[jj] = u.g;
            a.pg[jj] = u.pg;
            a.xi[jj] = u.xi;
            nn += u.pg * u.pg;
          }
        s[t] = nn;
      }
      a.partials[b] = lr_tree_host(s);
    }
  });
}

}  // namespace fdx
