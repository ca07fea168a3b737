// Stand-alone self-test of the TreeSHAP host twin (contrib_cpu.cpp) for sanitizer builds: a small
// hand-made ensemble against hand-computed values, including the empty row, a path without
// elements (d = 0) and a path at the depth limit (d = 32). Built with -fsanitize=address,undefined
// by fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("contrib"); exits non-zero on failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "contrib.h"
#include "ops.h"

using namespace fdx;

static int g_fail = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

struct Elem { int32_t feature; double z, lo, hi; };
struct Path { double v; std::vector<Elem> elems; };

// the path table of ops/text.py TreePaths, built the same way
struct Table {
  std::vector<int32_t> features, path_ptr, pe_slot, el_path, el_pos, slot_ptr, slot_blk, blk_slot;
  std::vector<double> path_v, pe_z, pe_lo, pe_hi, shapley;

  explicit Table(const std::vector<Path>& paths) {
    for (const Path& p : paths)
      for (const Elem& e : p.elems) features.push_back(e.feature);
    std::sort(features.begin(), features.end());
    features.erase(std::unique(features.begin(), features.end()), features.end());
    path_ptr.push_back(0);
    std::vector<int32_t> of_path;
    for (size_t p = 0; p < paths.size(); ++p) {
      path_v.push_back(paths[p].v);
      for (const Elem& e : paths[p].elems) {
        pe_slot.push_back((int32_t)(std::lower_bound(features.begin(), features.end(), e.feature) - features.begin()));
        pe_z.push_back(e.z), pe_lo.push_back(e.lo), pe_hi.push_back(e.hi);
        of_path.push_back((int32_t)p);
      }
      path_ptr.push_back((int32_t)pe_slot.size());
    }
    std::vector<int32_t> order(pe_slot.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pe_slot[a] < pe_slot[b]; });
    slot_ptr.assign(features.size() + 1, 0);
    for (int32_t e : order) {
      el_path.push_back(of_path[e]);
      el_pos.push_back(e - path_ptr[of_path[e]]);
      slot_ptr[pe_slot[e] + 1]++;
    }
    slot_blk.assign(features.size() + 1, 0);
    for (size_t s = 0; s < features.size(); ++s) {
      const int32_t nb = (slot_ptr[s + 1] + kContribBlockElems - 1) / kContribBlockElems;
      slot_ptr[s + 1] += slot_ptr[s];
      slot_blk[s + 1] = slot_blk[s] + nb;
      for (int32_t b = 0; b < nb; ++b) blk_slot.push_back((int32_t)s);
    }
    shapley.assign((kContribMaxDepth + 1) * kContribMaxDepth, 0.0);
    for (int d = 1; d <= kContribMaxDepth; ++d) {
      // w[d][0] = 1 / d; w[d][k] = w[d][k - 1] * k / (d - k)
      double w = 1.0 / d;
      for (int k = 0; k < d; ++k) {
        shapley[d * kContribMaxDepth + k] = w;
        w = w * (k + 1) / (d - k - 1 > 0 ? d - k - 1 : 1);
      }
    }
  }

  ContribPaths view(bool cmp_less) const {
    ContribPaths p{};
    p.features = features.data(), p.path_ptr = path_ptr.data(), p.path_v = path_v.data();
    p.pe_slot = pe_slot.data(), p.pe_z = pe_z.data(), p.pe_lo = pe_lo.data(), p.pe_hi = pe_hi.data();
    p.el_path = el_path.data(), p.el_pos = el_pos.data(), p.slot_ptr = slot_ptr.data();
    p.slot_blk = slot_blk.data(), p.blk_slot = blk_slot.data(), p.shapley = shapley.data();
    p.U = (int32_t)features.size(), p.P = (int32_t)path_v.size(), p.E = (int32_t)pe_slot.size();
    p.NB = (int32_t)blk_slot.size();
    p.cmp_less = cmp_less;
    return p;
  }
};

template <class V>
static std::vector<double> run(const Table& t, bool cmp_less, const std::vector<int64_t>& indptr,
                               const std::vector<int32_t>& idx, const std::vector<V>& val, int threads) {
  ContribArgs<V> a{};
  a.indptr = indptr.data(), a.idx = idx.data(), a.val = val.data();
  a.rows = (int64_t)indptr.size() - 1;
  a.p = t.view(cmp_less);
  std::vector<double> out((size_t)a.rows * t.features.size(), std::numeric_limits<double>::quiet_NaN());
  a.out = out.data();
  tree_contributions_cpu<V>(a, threads);
  return out;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  // One GBDT-style tree (go left iff x < threshold; covers in brackets):
  //   root [10]: f3 < 1.0 ? A : B        A [6]: f3 < 0.5 ? leaf 1.5 [2] : leaf -2.0 [4]
  //                                      B [4]: f5 < 2.0 ? leaf 0.7 [1] : leaf 3.0 [3]
  // then a single-leaf tree (0.25, a path without elements) and one path of 32 distinct features
  // (100..131), each with z = 0.5 and the test x >= 0.5, leaf value 1.
  std::vector<Path> paths = {
      {1.5, {{3, 0.6 * (2.0 / 6.0), -inf, 0.5}}},
      {-2.0, {{3, 0.6 * (4.0 / 6.0), 0.5, 1.0}}},
      {0.7, {{3, 0.4, 1.0, inf}, {5, 0.25, -inf, 2.0}}},
      {3.0, {{3, 0.4, 1.0, inf}, {5, 0.75, 2.0, inf}}},
      {0.25, {}},
      {1.0, {}},
  };
  for (int f = 0; f < 32; ++f) paths.back().elems.push_back({100 + f, 0.5, 0.5, inf});
  const Table t(paths);
  EXPECT(t.features.size() == 34 && t.blk_slot.size() == 34);

  // rows: {3: 0.2} | {3: 0.7, 5: 2.0} | empty | {1: 1, 3: 1.0, 5: 5.0} (x == threshold; 1 is unused) | all of 100..131
  std::vector<int64_t> indptr = {0, 1, 3, 3, 6};
  std::vector<int32_t> idx = {3, 3, 5, 1, 3, 5};
  std::vector<double> val = {0.2, 0.7, 2.0, 1.0, 1.0, 5.0};
  for (int f = 0; f < 32; ++f) idx.push_back(100 + f), val.push_back(1.0);
  indptr.push_back((int64_t)idx.size());

  // Shapley values of {f3, f5} from the conditional expectations v(S), e.g. row 0:
  // v() = 0.47, v(3) = 1.5, v(5) = -0.22, v(3,5) = 1.5 -> phi3 = (1.03 + 1.72) / 2, phi5 = (-0.69 + 0) / 2
  const double want[5][2] = {{1.375, -0.345}, {-2.585, 0.115}, {1.375, -0.345}, {2.1275, 0.4025}, {1.375, -0.345}};
  const double tiny = std::ldexp(1.0, -32);   // prod z of the 32-feature path
  const std::vector<double> out = run<double>(t, true, indptr, idx, val, 1);
  for (int r = 0; r < 5; ++r) {
    EXPECT(std::fabs(out[r * 34 + 0] - want[r][0]) < 1e-12);
    EXPECT(std::fabs(out[r * 34 + 1] - want[r][1]) < 1e-12);
    // by symmetry every feature of the long path gets (v o - v prod z) / 32
    const double each = ((r == 4 ? 1.0 : 0.0) - tiny) / 32.0;
    for (int s = 2; s < 34; ++s) EXPECT(std::fabs(out[r * 34 + s] - each) < 1e-12);
  }
  // thread count and value type change nothing (the values above are exact in float32 except 0.2 / 0.7,
  // which stay on their side of every threshold)
  const std::vector<double> out4 = run<double>(t, true, indptr, idx, val, 4);
  EXPECT(std::memcmp(out.data(), out4.data(), out.size() * sizeof(double)) == 0);
  const std::vector<float> valf(val.begin(), val.end());
  const std::vector<double> outf = run<float>(t, true, indptr, idx, valf, 3);
  EXPECT(std::memcmp(out.data(), outf.data(), out.size() * sizeof(double)) == 0);
  // the other comparison: x == threshold goes left (x <= 1.0), so row 3 lands in leaf -2.0
  const std::vector<double> le = run<double>(t, false, indptr, idx, val, 2);
  EXPECT(std::fabs(le[3 * 34 + 0] + le[3 * 34 + 1] + 0.47 - (-2.0)) < 1e-12);
  // no rows at all
  EXPECT(run<double>(t, true, {0}, {}, {}, 2).empty());

  if (g_fail) { std::fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
  std::puts("contrib selftest ok");
  return 0;
}
