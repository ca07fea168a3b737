// Host twins of the multi-class boosting kernels (contract in softprob.h). softprob_grad: every
// thread owns a range of rows and evaluates softprob_row_terms, as a lane does. score_class_trees:
// the lane order of the kernel, part[64][C] lane-strided partials and the same xor tree (lane 0 of
// the butterfly = halving adds), as text_cpu.cpp's class tail.
#include <stdexcept>

#include "parallel_for.h"
#include "softprob.h"

namespace fdx {

namespace {

template <int C>
void grad_c(const SoftprobGradArgs& a, int threads) {
  parallel_for(a.N, threads, 4096, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      double m[C];
      for (int c = 0; c < C; ++c) m[c] = a.margin[(int64_t)c * a.margin_stride + r];
      float g[C], h[C];
      softprob_row_terms<C>(m, a.y[r], a.w ? (double)a.w[r] : 1.0, g, h);
      for (int c = 0; c < C; ++c) {
        a.g[(int64_t)c * a.g_stride + r] = g[c];
        a.h[(int64_t)c * a.h_stride + r] = h[c];
      }
    }
  });
}

template <class V, int C>
void score_c(const ClassTreeArgs<V>& a, int threads) {
  parallel_for(a.rows, threads, 256, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t s = a.indptr[r], e = a.indptr[r + 1];
      const TreeEnsemble& te = a.trees;
      auto lookup = [&](int32_t f) -> double {
        int64_t l = s, h = e - 1;
        while (l <= h) {
          const int64_t m = (l + h) >> 1;
          if (a.idx[m] == f) return (double)a.val[m];
          if (a.idx[m] < f) l = m + 1; else h = m - 1;
        }
        return 0.0;
      };
      double part[kSoftprobWave][C] = {};
      for (int t = 0; t < te.num_trees; ++t) {
        const int32_t leaf = tree_find_leaf(te, te.roots[t], a.cmp_less, lookup);
        const double v = te.leaf[leaf];
        const int32_t k = a.tree_class[t];
        for (int c = 0; c < C; ++c) part[t & (kSoftprobWave - 1)][c] += (k == c) ? v : 0.0;
      }
      for (int o = kSoftprobWave / 2; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l)
          for (int c = 0; c < C; ++c) part[l][c] = part[l][c] + part[l + o][c];
      for (int c = 0; c < C; ++c) a.out[r * C + c] = part[0][c];
    }
  });
}

}  // namespace

void softprob_grad_cpu(const SoftprobGradArgs& a, int threads) {
  if (a.N <= 0) return;
  switch (a.num_classes) {
    case 2: grad_c<2>(a, threads); break;
    case 3: grad_c<3>(a, threads); break;
    case 4: grad_c<4>(a, threads); break;
    case 5: grad_c<5>(a, threads); break;
    case 6: grad_c<6>(a, threads); break;
    case 7: grad_c<7>(a, threads); break;
    case 8: grad_c<8>(a, threads); break;
    default: throw std::runtime_error("fdx softprob_grad: classes out of range");
  }
}

template <class V>
void score_class_trees_cpu(const ClassTreeArgs<V>& a, int threads) {
  if (a.rows <= 0) return;
  switch (a.num_classes) {
    case 2: score_c<V, 2>(a, threads); break;
    case 3: score_c<V, 3>(a, threads); break;
    case 4: score_c<V, 4>(a, threads); break;
    case 5: score_c<V, 5>(a, threads); break;
    case 6: score_c<V, 6>(a, threads); break;
    case 7: score_c<V, 7>(a, threads); break;
    case 8: score_c<V, 8>(a, threads); break;
    default: throw std::runtime_error("fdx score_class_trees: classes out of range");
  }
}
template void score_class_trees_cpu<float>(const ClassTreeArgs<float>&, int);
template void score_class_trees_cpu<double>(const ClassTreeArgs<double>&, int);

}  // namespace fdx
