// Host twin of contrib_kernels.hip: the same terms (contrib.h) in the same summation order (stated
// at the top of the kernel file), rows spread over the host pool. Every row is computed by one
// thread from the inputs alone, so the result does not depend on the thread count.
#include <vector>

#include "contrib.h"
#include "ops.h"
#include "parallel_for.h"

namespace fdx {

template <class V>
void tree_contributions_cpu(const ContribArgs<V>& a, int threads) {
  const ContribPaths& t = a.p;
  if (t.U <= 0) return;
  parallel_for(a.rows, threads, 8, [&](int64_t lo, int64_t hi) {
    std::vector<double> xs((size_t)t.U);
    std::vector<uint32_t> masks((size_t)t.P);
    for (int64_t r = lo; r < hi; ++r) {
      std::fill(xs.begin(), xs.end(), 0.0);
      for (int64_t j = a.indptr[r]; j < a.indptr[r + 1]; ++j) {
        const int32_t s = sorted_find(t.features, t.U, a.idx[j]);
        if (s >= 0) xs[(size_t)s] = (double)a.val[j];
      }
      for (int32_t p = 0; p < t.P; ++p) {
        uint32_t mask = 0;
        const int32_t e0 = t.path_ptr[p], e1 = t.path_ptr[p + 1];
        for (int32_t e = e0; e < e1; ++e)
          if (contrib_test(xs[(size_t)t.pe_slot[e]], t.pe_lo[e], t.pe_hi[e], t.cmp_less)) mask |= 1u << (e - e0);
        masks[(size_t)p] = mask;
      }
      double* out = a.out + r * t.U;
      for (int32_t s = 0; s < t.U; ++s) {
        double total = 0.0;
        for (int32_t e0 = t.slot_ptr[s], first = e0; e0 < t.slot_ptr[s + 1]; e0 += kContribBlockElems) {
          const int32_t e1 = e0 + kContribBlockElems < t.slot_ptr[s + 1] ? e0 + kContribBlockElems : t.slot_ptr[s + 1];
          double acc = 0.0;
          for (int32_t e = e0; e < e1; ++e) {
            const int32_t p = t.el_path[e];
            const int32_t q = t.path_ptr[p];
            acc += contrib_term(t.pe_z + q, t.path_ptr[p + 1] - q, masks[(size_t)p], t.el_pos[e], t.shapley,
                                t.path_v[p]);
          }
          total = e0 == first ? acc : total + acc;
        }
        out[s] = total;
      }
    }
  });
}
template void tree_contributions_cpu<float>(const ContribArgs<float>&, int);
template void tree_contributions_cpu<double>(const ContribArgs<double>&, int);

}  // namespace fdx
