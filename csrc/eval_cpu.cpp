// Host twins of eval_kernels.hip: the same per-element code (eval.h), integer sums (any thread
// count gives the same bits), rows spread over the host pool.
#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

#include "eval.h"
#include "ops.h"
#include "parallel_for.h"

namespace fdx {

template <class V>
void tree_eval_update_cpu(const TreeEvalArgs<V>& a, int threads) {
  const EvalTree& t = a.t;
  parallel_for(a.rows, threads, 256, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; ++r) {
      const int64_t b = a.indptr[r];
      const int32_t len = (int32_t)(a.indptr[r + 1] - b);
      int32_t n = 0;
      for (int guard = 0; guard < kEvalMaxWalk && eval_is_inner(t, n); ++guard) {
        const int32_t j = sorted_find(a.idx + b, len, (int32_t)t.fid_orig[t.feat[n]]);
        const int32_t c = eval_next(t, n, j >= 0 ? (double)a.val[b + j] : 0.0);
        if (c < 0) break;
        n = c;
      }
      a.margin[r] += eval_leaf(t, n);
    }
  });
}
template void tree_eval_update_cpu<float>(const TreeEvalArgs<float>&, int);
template void tree_eval_update_cpu<double>(const TreeEvalArgs<double>&, int);

void eval_sums_cpu(const EvalSumArgs& a, int threads) {
  std::atomic<int64_t> sl{0}, se{0}, sw{0};
  parallel_for(a.n, threads, 1024, [&](int64_t lo, int64_t hi) {
    int64_t l = 0, e = 0, w = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const EvalTerms t = eval_terms(a.margin[i], a.label[i], a.weight ? (double)a.weight[i] : 1.0, a.scale);
      l += t.l;
      e += t.e;
      w += t.w;
    }
    sl.fetch_add(l, std::memory_order_relaxed);
    se.fetch_add(e, std::memory_order_relaxed);
    sw.fetch_add(w, std::memory_order_relaxed);
  });
  a.out[0] += sl.load();
  a.out[1] += se.load();
  a.out[2] += sw.load();
}

void eval_auc_cpu(const double* margin, const float* label, int64_t n, int64_t* out) {
  std::vector<std::pair<uint64_t, uint8_t>> v((size_t)n);
  for (int64_t i = 0; i < n; ++i) v[(size_t)i] = {eval_auc_key(margin[i]), (uint8_t)(label[i] > 0.5f ? 1 : 0)};
  std::sort(v.begin(), v.end());
  int64_t u2 = 0, pos = 0, neg_before = 0;
  for (size_t s = 0; s < v.size();) {
    size_t e = s;
    int64_t rp = 0, rn = 0;                 // positives / negatives of the run of equal keys
    for (; e < v.size() && v[e].first == v[s].first; ++e) (v[e].second ? rp : rn) += 1;
    u2 += rp * (2 * neg_before + rn);
    pos += rp;
    neg_before += rn;
    s = e;
  }
  out[0] = u2;
  out[1] = pos;
  out[2] = neg_before;
}

}  // namespace fdx
