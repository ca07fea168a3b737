// Stand-alone self-test of the Naive Bayes host twins (nb_cpu.cpp) for sanitizer builds: rows of
// 0, 1, 63, 64, 65 and 129 entries, 2, 3 and 8 classes (one of them without rows), fp32 and fp64
// values, unit and non-dyadic weights, 1, 4 and 7 threads; every buffer is sized exactly, so a read
// or write past a row, a class or the feature space is caught. Sums are compared with a direct
// evaluation of the contract and across the thread counts, scores bit for bit with the lane-order
// sum; bad labels, weights, values and feature ids must set the flag word and add nothing.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("nb"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "nb.h"

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <class V>
struct Data {
  int F, C;
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  std::vector<double> y, w;
  int64_t rows() const { return (int64_t)y.size(); }
  void add_row(int len, int label, double weight, bool counts) {
    std::vector<int32_t> ids(F);
    std::iota(ids.begin(), ids.end(), 0);
    for (int i = 0; i < len; ++i) std::swap(ids[i], ids[i + (int)(rnd64() % (uint64_t)(F - i))]);
    for (int i = 0; i < len; ++i) {
      idx.push_back(ids[i]);
      val.push_back(counts ? (V)(1 + rnd64() % 5) : (V)(0.1 + 2.9 * rnd()));
    }
    indptr.push_back((int64_t)idx.size());
    y.push_back(label);
    w.push_back(weight);
  }
};

template <class V>
static std::vector<int64_t> run_sums(const Data<V>& d, bool weighted, bool bernoulli, int k, int kw, int threads) {
  std::vector<int64_t> out((size_t)d.C * d.F + 2 * d.C + 1, 0);
  NbSumArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.labels = d.y.data(); a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = d.F; a.num_classes = d.C; a.k = k; a.kw = kw; a.bernoulli = bernoulli;
  a.S = out.data(); a.Wq = a.S + (int64_t)d.C * d.F; a.cnt = a.Wq + d.C; a.flag = a.cnt + d.C;
  nb_sums_cpu<V>(a, threads);
  return out;
}

template <class V>
static std::vector<int64_t> direct_sums(const Data<V>& d, bool weighted, int k, int kw) {
  std::vector<int64_t> out((size_t)d.C * d.F + 2 * d.C + 1, 0);
  for (int64_t r = 0; r < d.rows(); ++r) {
    const int c = (int)d.y[r];
    const double w = weighted ? d.w[r] : 1.0;
    out[(size_t)d.C * d.F + c] += (int64_t)std::nearbyint(std::ldexp(w, kw));
    out[(size_t)d.C * d.F + d.C + c] += 1;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j)
      out[(size_t)c * d.F + d.idx[j]] += (int64_t)std::nearbyint(std::ldexp(w * (double)d.val[j], k));
  }
  return out;
}

template <class V>
static Data<V> make(int C, int extra_rows, bool counts) {
  Data<V> d;
  d.F = 300;
  d.C = C;
  const int empty = C - 1;                       // the last class has no rows
  auto label = [&] { return (int)(rnd64() % (uint64_t)(empty > 0 ? empty : 1)); };
  for (int len : {0, 1, 63, 64, 65, 129, 0, 17}) d.add_row(len, label(), 0.3 + 1.7 * rnd(), counts);
  for (int i = 0; i < extra_rows; ++i) d.add_row((int)(rnd64() % 40), label(), 0.3 + 1.7 * rnd(), counts);
  return d;
}

template <class V>
static void test_sums(int C) {
  for (bool counts : {true, false}) {
    const Data<V> d = make<V>(C, 2100, counts);
    for (bool weighted : {false, true}) {
      const int k = 30, kw = 35;
      const std::vector<int64_t> want = direct_sums(d, weighted, k, kw);
      EXPECT(want.back() == 0 && want[(size_t)d.C * d.F + 2 * d.C - 1] == 0);
      for (int threads : {1, 4, 7}) EXPECT(run_sums(d, weighted, false, k, kw, threads) == want);
      if (counts && !weighted) {                 // S 2^-k is the exact count sum
        int64_t total = 0, ref = 0;
        for (int64_t i = 0; i < (int64_t)d.C * d.F; ++i) total += want[i] >> k;
        for (const V v : d.val) ref += (int64_t)v;
        EXPECT(total == ref);
      }
    }
  }
}

static void test_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Data<double> base = make<double>(3, 40, true);
  const std::vector<int64_t> clean = run_sums(base, true, false, 20, 20, 1);
  EXPECT(clean.back() == 0);
  auto flagged = [&](const Data<double>& d, bool bernoulli) { return run_sums(d, true, bernoulli, 20, 20, 4).back() == 1; };
  for (double bad : {-1.0, 0.5, 3.0, nan, inf}) { Data<double> d = base; d.y[5] = bad; EXPECT(flagged(d, false)); }
  for (double bad : {0.0, -2.0, nan, inf}) { Data<double> d = base; d.w[5] = bad; EXPECT(flagged(d, false)); }
  for (double bad : {-0.5, nan, inf}) { Data<double> d = base; d.val[70] = bad; EXPECT(flagged(d, false)); }
  { Data<double> d = base; d.idx[70] = d.F; EXPECT(flagged(d, false)); }
  { Data<double> d = base; d.idx[70] = -1; EXPECT(flagged(d, false)); }
  EXPECT(flagged(base, true));                   // counts above 1 are no Bernoulli input
  Data<double> ones = base;
  for (double& v : ones.val) v = 1.0;
  EXPECT(!flagged(ones, true));
  EXPECT(nb_label(2.0, 3) == 2 && nb_label(3.0, 3) == -1 && nb_label(-0.0, 3) == 0 && nb_label(1.5, 3) == -1);
  EXPECT(nb_quant(0.5, 0) == 0 && nb_quant(1.5, 0) == 2 && nb_quant(2.5, 0) == 2 && nb_quant(0.75, 2) == 3);
}

template <class V>
static void test_score(int C) {
  const Data<V> d = make<V>(C, 1100, false);
  std::vector<double> W((size_t)d.F * C), b(C);
  for (double& x : W) x = -12.0 * rnd();
  for (double& x : b) x = -3.0 * rnd();
  std::vector<double> ref;
  for (int threads : {1, 4}) {
    std::vector<double> out((size_t)d.rows() * C);
    NbScoreArgs<V> a{d.indptr.data(), d.idx.data(), d.val.data(), d.rows(), d.F, C, W.data(), b.data(), out.data()};
    nb_score_cpu<V>(a, threads);
    if (ref.empty()) {
      ref = out;
      for (int64_t r = 0; r < d.rows(); ++r)
        for (int c = 0; c < C; ++c) {
          double p[kNbWave] = {0};
          for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j)
            p[(j - d.indptr[r]) & (kNbWave - 1)] += (double)d.val[j] * W[(size_t)d.idx[j] * C + c];
          EXPECT(same_bits(out[r * C + c], nb_butterfly_host(p) + b[c]));
        }
    } else {
      EXPECT(std::memcmp(ref.data(), out.data(), out.size() * sizeof(double)) == 0);
    }
  }
}

int main() {
  for (int C : {2, 3, kNbMaxClasses}) {
    test_sums<double>(C);
    test_sums<float>(C);
    test_score<double>(C);
    test_score<float>(C);
  }
  test_flags();
  if (g_fail) {
    std::fprintf(stderr, "nb_selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("nb_selftest: ok\n");
  return 0;
}
