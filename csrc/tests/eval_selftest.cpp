// Stand-alone self-test of the validation-monitoring host twins (eval_cpu.cpp) for sanitizer
// builds: a hand-made node table over rows with absent features, an empty row, a value exactly on
// a threshold and a malformed table; the fixed-point sums and the AUC integers against values
// computed by hand, including ties, signed zeros, a one-class set and the empty set. Built with
// -fsanitize=address,undefined by fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("eval");
// exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <vector>

#include "eval.h"
#include "ops.h"

using namespace fdx;

static int g_fail = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static void test_tree_update() {
  // node 0: active feature 1 (original 7), bin 1 -> threshold 0.5; node 1: active feature 0
  // (original 2), bin 0 -> threshold -1.0; leaves 2, 3, 4
  std::vector<int32_t> feat = {1, 0, -1, -1, -1, -1, -1, -1}, bin = {1, 0, -1, -1, -1, -1, -1, -1};
  std::vector<int32_t> left = {1, 3, -1, -1, -1, -1, -1, -1}, right = {2, 4, -1, -1, -1, -1, -1, -1};
  std::vector<uint8_t> leaf = {0, 0, 1, 1, 1, 0, 0, 0};
  std::vector<int64_t> stats(16, 0);
  const int64_t g[5] = {0, 0, -8, 4, 16}, h[5] = {0, 0, 6, 2, 14};
  for (int n = 0; n < 5; ++n) stats[2 * n] = g[n], stats[2 * n + 1] = h[n];
  std::vector<int32_t> kexp = {2, 1};                      // G = g / 4, H = h / 2
  std::vector<int64_t> fid_orig = {2, 7}, boff = {0, 1, 3};
  std::vector<double> thr = {-1.0, 0.25, 0.5};
  EvalTree t{};
  t.feat = feat.data(), t.bin = bin.data(), t.left = left.data(), t.right = right.data(), t.leaf = leaf.data();
  t.stats = stats.data(), t.kexp = kexp.data(), t.fid_orig = fid_orig.data(), t.boff = boff.data();
  t.thresholds = thr.data(), t.max_nodes = 8, t.Fa = 2, t.TB = 3, t.eta = 0.5, t.lambda = 1.0, t.mds = 0.0;
  // leaf values: eta * -G / (H + 1): node 2: 0.5 * 2 / 4 = 0.25; node 3: 0.5 * -1 / 2 = -0.25; node 4: 0.5 * -4 / 8 = -0.25
  // rows: {} -> 7 absent (0 < 0.5 left), 2 absent (0 < -1 false) -> node 4
  //       {7: 0.5} -> on the threshold: right -> node 2
  //       {2: -3, 7: 0.1} -> left, left -> node 3
  //       {1: 9, 2: -1, 9: 1} -> 7 absent: left; -1 < -1 false -> node 4
  std::vector<int64_t> indptr = {0, 0, 1, 3, 6};
  std::vector<int32_t> idx = {7, 2, 7, 1, 2, 9};
  std::vector<float> val = {0.5f, -3.f, 0.1f, 9.f, -1.f, 1.f};
  for (int threads : {1, 3}) {
    std::vector<double> margin(4, 1.0);
    TreeEvalArgs<float> a{indptr.data(), idx.data(), val.data(), 4, t, margin.data()};
    tree_eval_update_cpu<float>(a, threads);
    EXPECT(margin[0] == 0.75 && margin[1] == 1.25 && margin[2] == 0.75 && margin[3] == 0.75);
  }
  // a malformed table (child outside the table, feature outside the map) ends the walk at the node
  right[0] = 99;
  feat[1] = 5;
  std::vector<double> margin(4, 0.0);
  TreeEvalArgs<float> a{indptr.data(), idx.data(), val.data(), 4, t, margin.data()};
  tree_eval_update_cpu<float>(a, 1);
  EXPECT(std::isfinite(margin[0]) && std::isfinite(margin[1]));
}

static void test_sums() {
  EXPECT(eval_sum_kexp(1, 1.0) == 40 && eval_sum_kexp(1 << 20, 1.0) == 36 && eval_sum_kexp(1 << 20, 4.0) == 34);
  EXPECT(eval_sum_kexp((1 << 20) + 1, 3.5) == 33);
  std::vector<double> m = {0.0, 2.0, -2.0, 800.0, -800.0};
  std::vector<float> y = {1.f, 0.f, 0.f, 0.f, 1.f}, w = {1.f, 0.5f, 2.f, 1.f, 0.25f};
  int64_t out[3] = {0, 0, 0};
  const int k = 30;
  EvalSumArgs a{m.data(), y.data(), w.data(), 5, std::ldexp(1.0, k), out};
  eval_sums_cpu(a, 2);
  // errors: m = 0 with y = 1 (p = 0.5 is not > 0.5), m = 2 with y = 0, and both saturated rows
  EXPECT(out[1] == (int64_t)std::llrint((1.0 + 0.5 + 1.0 + 0.25) * std::ldexp(1.0, k)));
  EXPECT(out[2] == (int64_t)std::llrint(4.75 * std::ldexp(1.0, k)));
  const double cap = -std::log(1e-16);
  const double want = std::log(2.0) + 0.5 * std::log1p(std::exp(2.0)) + 2.0 * std::log1p(std::exp(-2.0)) + cap + 0.25 * cap;
  EXPECT(std::fabs((double)out[0] * std::ldexp(1.0, -k) - want) < 1e-8);
  int64_t none[3] = {0, 0, 0};
  EvalSumArgs e{m.data(), y.data(), nullptr, 0, 1.0, none};
  eval_sums_cpu(e, 0);
  EXPECT(none[0] == 0 && none[2] == 0);
}

static void test_auc() {
  EXPECT(eval_auc_key(-0.0) == eval_auc_key(0.0));
  EXPECT(eval_auc_key(-1.0) < eval_auc_key(-0.5) && eval_auc_key(-0.5) < eval_auc_key(0.0) &&
         eval_auc_key(0.0) < eval_auc_key(1e-300) && eval_auc_key(1.0) < eval_auc_key(INFINITY));
  // sorted: -1(n) | -0,+0: (p, n) | 0.5 (p) | 2, 2, 2: (n, p, p)
  std::vector<double> m = {2.0, 0.0, -1.0, 2.0, 0.5, -0.0, 2.0};
  std::vector<float> y = {1.f, 1.f, 0.f, 0.f, 1.f, 0.f, 1.f};
  int64_t out[3];
  eval_auc_cpu(m.data(), y.data(), 7, out);
  // U2 = (2 * 1 + 1) + (2 * 2) + 2 * (2 * 2 + 1) = 17
  EXPECT(out[0] == 17 && out[1] == 4 && out[2] == 3);
  std::vector<float> ones(7, 1.f);
  eval_auc_cpu(m.data(), ones.data(), 7, out);
  EXPECT(out[0] == 0 && out[1] == 7 && out[2] == 0);
  eval_auc_cpu(m.data(), y.data(), 0, out);
  EXPECT(out[0] == 0 && out[1] == 0 && out[2] == 0);
}

int main() {
  test_tree_update();
  test_sums();
  test_auc();
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("eval selftest ok\n");
  return 0;
}
