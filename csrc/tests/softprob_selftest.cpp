// Stand-alone self-test of the multi-class boosting host twins (softprob_cpu.cpp) for sanitizer
// builds. softprob_grad: 1, 63, 64, 65, 257, 4097 and 9001 rows, 2, 3 and 8 classes, with and without
// weights (0 among them), margins forced to +-40 and +-700 in one class, planes that are strided
// views of a sentinel-filled buffer (the sentinels must survive, every [c, :N] must be written), and
// 1, 4 and 7 threads giving the same bits. score_class_trees: depth-3 trees over 40 features, 2, 3 and
// 63 .. 193 trees, rows of 0, 1 and 65 entries, fp32 and fp64 values, both comparison modes, class ids
// round robin and shuffled with one class owning no tree (its column is +0.0 bit for bit), checked
// against a direct lane-order evaluation. Every buffer is sized exactly, so a read or write past a
// row, a plane or the tree list is caught.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("softprob"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "softprob.h"

using namespace fdx;

static int g_fail = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() {      // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545f4914f6cdd1dull;
}
static double rnd() { return (double)(rnd64() >> 11) * (1.0 / 9007199254740992.0); }

static void test_grad(int C, int64_t N, bool weighted) {
  const float kSent = -12345.0f;
  const int64_t stride = N + 64;
  std::vector<double> m((size_t)C * N);
  std::vector<float> y((size_t)N), w((size_t)N);
  for (double& v : m) v = 6.0 * rnd() - 3.0;
  for (int64_t r = 0; r < N; ++r) {
    y[r] = (float)(rnd64() % (uint64_t)C);
    w[r] = r % 7 == 3 ? 0.0f : (float)(0.1 + 2.9 * rnd());
  }
  const double forced[4] = {40.0, -40.0, 700.0, -700.0};
  for (int64_t r = 0; r < N && r < 8; ++r) m[(size_t)(r % C) * N + r] = forced[r % 4];
  auto run = [&](int threads) {
    std::vector<float> buf((size_t)2 * C * stride, kSent);
    SoftprobGradArgs a{};
    a.margin = m.data(); a.margin_stride = N;
    a.y = y.data(); a.w = weighted ? w.data() : nullptr;
    a.g = buf.data(); a.g_stride = stride;
    a.h = buf.data() + (size_t)C * stride; a.h_stride = stride;
    a.N = N; a.num_classes = C;
    softprob_grad_cpu(a, threads);
    return buf;
  };
  const std::vector<float> ref = run(1);
  for (int threads : {4, 7}) EXPECT(run(threads) == ref);
  const float floor_h = (float)kSoftprobMinHess;
  for (int64_t r = 0; r < N; ++r) {
    const double wr = weighted ? (double)w[r] : 1.0;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
      const float g = ref[(size_t)c * stride + r], h = ref[(size_t)(C + c) * stride + r];
      EXPECT(g != kSent && h != kSent);
      EXPECT((float)c == y[r] ? g <= 0.0f : g >= 0.0f);
      EXPECT(h >= floor_h && std::fabs((double)g) <= wr);
      if (wr == 0.0) EXPECT(g == 0.0f && h == floor_h);
      sum += g;
    }
    EXPECT(std::fabs(sum) <= 1e-6 * wr * C);
  }
  for (int p = 0; p < 2 * C; ++p)
    for (int64_t r = N; r < stride; ++r) EXPECT(ref[(size_t)p * stride + r] == kSent);
}

struct Forest {
  std::vector<int32_t> feat, left, right, roots, cls;
  std::vector<double> thr, leaf;
};

// complete depth-3 trees over F features
static Forest make_forest(int T, int C, int F, bool shuffled) {
  Forest f;
  for (int t = 0; t < T; ++t) {
    const int32_t base = (int32_t)f.feat.size();
    f.roots.push_back(base);
    for (int i = 0; i < 15; ++i) {
      const bool internal = i < 7;
      f.feat.push_back(internal ? (int32_t)(rnd64() % (uint64_t)F) : -1);
      f.thr.push_back(internal ? 4.0 * rnd() - 1.0 : 0.0);
      f.left.push_back(internal ? base + 2 * i + 1 : -1);
      f.right.push_back(internal ? base + 2 * i + 2 : -1);
      f.leaf.push_back(internal ? 0.0 : 2.0 * rnd() - 1.0);
    }
    // shuffled: any class but the last, which then owns no tree
    f.cls.push_back(shuffled ? (int32_t)(rnd64() % (uint64_t)(C - 1)) : t % C);
  }
  return f;
}

template <class V>
static void test_score(int T, int C, bool shuffled, bool cmp_less) {
  const int F = 40;
  const Forest f = make_forest(T, C, F, shuffled);
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  for (int len : {0, 1, 65, 7, 40, 0, 13}) {
    // (65 stored entries: ids run past the 40 features the trees read, ascending)
    const int step = len ? (len > F ? 2 : F / len) : 1;
    for (int i = 0; i < len; ++i) {
      idx.push_back(i * step + (int32_t)(rnd64() % (uint64_t)step));
      val.push_back((V)(4.0 * rnd() - 1.0));
    }
    indptr.push_back((int64_t)idx.size());
  }
  const int64_t rows = (int64_t)indptr.size() - 1;
  auto run = [&](int threads) {
    std::vector<double> out((size_t)rows * C, -7.0);
    ClassTreeArgs<V> a{};
    a.indptr = indptr.data(); a.idx = idx.data(); a.val = val.data(); a.rows = rows;
    a.trees.feat = f.feat.data(); a.trees.thr = f.thr.data(); a.trees.left = f.left.data();
    a.trees.right = f.right.data(); a.trees.leaf = f.leaf.data(); a.trees.roots = f.roots.data();
    a.trees.num_trees = T; a.trees.K = 1;
    a.tree_class = f.cls.data(); a.num_classes = C; a.cmp_less = cmp_less; a.out = out.data();
    score_class_trees_cpu<V>(a, threads);
    return out;
  };
  const std::vector<double> got = run(1);
  EXPECT(run(7) == got);
  for (int64_t r = 0; r < rows; ++r) {
    std::vector<double> part((size_t)64 * C, 0.0);
    for (int t = 0; t < T; ++t) {
      int32_t n = f.roots[t];
      while (f.feat[n] >= 0) {
        double x = 0.0;
        for (int64_t j = indptr[r]; j < indptr[r + 1]; ++j)
          if (idx[j] == f.feat[n]) x = (double)val[j];
        n = (cmp_less ? x < f.thr[n] : x <= f.thr[n]) ? f.left[n] : f.right[n];
      }
      part[(size_t)(t & 63) * C + f.cls[t]] += f.leaf[n];
    }
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l)
        for (int c = 0; c < C; ++c) part[(size_t)l * C + c] += part[(size_t)(l + o) * C + c];
    EXPECT(std::memcmp(part.data(), &got[(size_t)r * C], sizeof(double) * C) == 0);
    if (shuffled) {
      const double z = got[(size_t)r * C + C - 1];
      EXPECT(z == 0.0 && !std::signbit(z));
    }
  }
}

int main() {
  for (int C : {2, 3, kSoftprobMaxClasses})
    for (int64_t N : {1, 63, 64, 65, 257, 4097, 9001})
      for (bool weighted : {false, true}) test_grad(C, N, weighted);
  for (int C : {2, 3, kSoftprobMaxClasses})
    for (int T : {C, 63, 64, 65, 129, 193})
      for (bool shuffled : {false, true})
        for (bool less : {false, true}) {
          test_score<double>(T, C, shuffled, less);
          test_score<float>(T, C, shuffled, less);
        }
  if (g_fail) {
    std::fprintf(stderr, "softprob selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("softprob selftest ok\n");
  return 0;
}
