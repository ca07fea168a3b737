// Stand-alone self-test of the multinomial logistic-regression host twin (mlr_cpu.cpp) for sanitizer
// builds: rows of 0, 1, 63, 64, 65 and 129 entries, 2, 3 and 8 classes, fp32 and fp64 values, unit
// weights and weights from {0.5, 3}, negative values, forced margins of +-40, +-800 and 5000, and 1, 4
// and 7 threads; every buffer is sized exactly, so a read or write past a row, a class or the feature
// space is caught. Margins are compared bit for bit with nb_score_cpu, the block with a direct
// integer evaluation of the contract on the twin's own residuals and across the thread counts; bad
// labels, weights, values and feature ids must set the high half of the flag word and add nothing,
// and no value that is not finite may reach a conversion to an integer.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("mlr"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "mlr.h"

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

template <class V>
struct Data {
  int F = 300, C = 3;
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  std::vector<double> y, w, XS, b;
  int64_t rows() const { return (int64_t)y.size(); }
  void add_row(int len, int label, double weight) {
    std::vector<int32_t> ids(F - 5);
    std::iota(ids.begin(), ids.end(), 5);          // features 0 .. 4 carry the forced margins
    for (int i = 0; i < len; ++i) std::swap(ids[i], ids[i + (int)(rnd64() % (uint64_t)(F - 5 - i))]);
    for (int i = 0; i < len; ++i) {
      idx.push_back(ids[i]);
      val.push_back((V)((rnd() < 0.15 ? -1.0 : 1.0) * (0.1 + 2.9 * rnd())));
    }
    indptr.push_back((int64_t)idx.size());
    y.push_back(label);
    w.push_back(weight);
  }
  void add_forced(int feature, int label, double weight) {
    idx.push_back(feature);
    val.push_back((V)1);
    indptr.push_back((int64_t)idx.size());
    y.push_back(label);
    w.push_back(weight);
  }
};

template <class V>
static Data<V> make(int C, int extra_rows, bool with_5000) {
  Data<V> d;
  d.C = C;
  auto label = [&] { return (int)(rnd64() % (uint64_t)C); };
  auto weight = [&] { return rnd() < 0.5 ? 0.5 : 3.0; };
  for (int len : {0, 1, 63, 64, 65, 129, 0, 17}) d.add_row(len, label(), weight());
  for (int f = 0; f < (with_5000 ? 5 : 4); ++f) d.add_forced(f, f == 4 ? 1 : label(), weight());
  for (int i = 0; i < extra_rows; ++i) d.add_row((int)(rnd64() % 40), label(), weight());
  d.XS.resize((size_t)d.F * C);
  d.b.resize(C);
  for (double& x : d.XS) x = 0.8 * rnd() - 0.4;
  for (double& x : d.b) x = rnd() - 0.5;
  const double forced[5] = {40.0, -40.0, 800.0, -800.0, 5000.0};
  for (int f = 0; f < 5; ++f)
    for (int c = 0; c < C; ++c) d.XS[(size_t)f * C + c] = c == 0 ? forced[f] : 0.0;
  return d;
}

template <class V>
struct Out {
  std::vector<int64_t> block;
  std::vector<double> margin, R, loss;
};

template <class V>
static Out<V> run(const Data<V>& d, bool weighted, int k, int kl, int threads, bool rows) {
  Out<V> o;
  o.block.assign((size_t)d.F * d.C + d.C + 2, 0);
  if (rows) {
    o.margin.assign((size_t)d.rows() * d.C, -1.0);
    o.R.assign((size_t)d.rows() * d.C, -1.0);
    o.loss.assign((size_t)d.rows(), -1.0);
  }
  MlrArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.XS = d.XS.data(); a.b = d.b.data();
  a.labels = d.y.data(); a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = d.F; a.num_classes = d.C; a.k = k; a.kl = kl;
  a.Gq = o.block.data(); a.gbq = a.Gq + (int64_t)d.F * d.C; a.lossq = a.gbq + d.C; a.flag = a.lossq + 1;
  a.margin = rows ? o.margin.data() : nullptr;
  a.R = rows ? o.R.data() : nullptr;
  a.loss_row = rows ? o.loss.data() : nullptr;
  mlr_eval_cpu<V>(a, threads);
  return o;
}

// the block from the twin's own residuals and losses, by the contract
template <class V>
static std::vector<int64_t> direct(const Data<V>& d, bool weighted, const Out<V>& o, int k, int kl) {
  const int C = d.C;
  std::vector<int64_t> out((size_t)d.F * C + C + 2, 0);
  for (int64_t r = 0; r < d.rows(); ++r) {
    const double w = weighted ? d.w[r] : 1.0;
    out[(size_t)d.F * C + C] += (int64_t)std::nearbyint(std::ldexp(w * o.loss[r], kl));
    for (int c = 0; c < C; ++c) {
      out[(size_t)d.F * C + c] += (int64_t)std::nearbyint(std::ldexp(o.R[r * C + c], k));
      for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j)
        out[(size_t)d.idx[j] * C + c] += (int64_t)std::nearbyint(std::ldexp((double)d.val[j] * o.R[r * C + c], k));
    }
  }
  return out;
}

template <class V>
static void test_eval(int C) {
  const Data<V> d = make<V>(C, 2100, false);
  for (bool weighted : {false, true}) {
    const int k = 38, kl = 36;
    const Out<V> ref = run(d, weighted, k, kl, 1, true);
    EXPECT(ref.block.back() == 0);
    EXPECT(ref.block == direct(d, weighted, ref, k, kl));
    for (int threads : {4, 7}) {
      EXPECT(run(d, weighted, k, kl, threads, false).block == ref.block);
      const Out<V> again = run(d, weighted, k, kl, threads, true);
      EXPECT(again.block == ref.block && again.R == ref.R && again.loss == ref.loss && again.margin == ref.margin);
    }
    // margins: bit for bit the class scores
    std::vector<double> score((size_t)d.rows() * C);
    NbScoreArgs<V> s{d.indptr.data(), d.idx.data(), d.val.data(), d.rows(), d.F, C, d.XS.data(), d.b.data(), score.data()};
    nb_score_cpu<V>(s, 3);
    EXPECT(std::memcmp(score.data(), ref.margin.data(), score.size() * sizeof(double)) == 0);
    // row terms: probabilities sum to the label's share, losses are finite and below the cap
    for (int64_t r = 0; r < d.rows(); ++r) {
      const double w = weighted ? d.w[r] : 1.0;
      double sum = 0.0;
      for (int c = 0; c < C; ++c) {
        EXPECT(std::fabs(ref.R[r * C + c]) <= w);
        sum += ref.R[r * C + c];
      }
      EXPECT(std::fabs(sum) <= 1e-15 * w * C);
      EXPECT(ref.loss[r] >= 0.0 && ref.loss[r] < kMlrLossCap);
    }
  }
}

static void test_clamp() {
  const double inf = std::numeric_limits<double>::infinity();
  Data<double> d = make<double>(3, 40, true);
  const int64_t row = 8 + 4;                     // the row of feature 4: margin 5000 for class 0, label 1
  Out<double> o = run(d, true, 30, 28, 4, true);
  EXPECT(o.block.back() == kMlrFlagClamped);
  EXPECT(o.loss[row] == kMlrLossCap && o.R[row * 3] == d.w[row] && o.R[row * 3 + 1] == -d.w[row] && o.R[row * 3 + 2] == 0.0);
  EXPECT(o.block == [&] { auto v = direct(d, true, o, 30, 28); v.back() = kMlrFlagClamped; return v; }());
  for (double bad : {inf, std::numeric_limits<double>::quiet_NaN()}) {
    Data<double> e = d;
    e.XS[4 * 3] = bad;                           // a margin that is not finite: clamped, no residual
    const Out<double> p = run(e, true, 30, 28, 1, true);
    EXPECT(p.block.back() == kMlrFlagClamped && p.loss[row] == kMlrLossCap);
    EXPECT(p.R[row * 3] == 0.0 && p.R[row * 3 + 1] == 0.0 && p.R[row * 3 + 2] == 0.0);
  }
}

static void test_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Data<double> base = make<double>(3, 300, false);
  const int64_t row = 20, at = base.indptr[row];
  EXPECT(base.indptr[row + 1] > at);
  EXPECT(run(base, true, 20, 20, 1, false).block.back() == 0);
  Data<double> gone = base;
  gone.w[row] = 0.0;                             // a row of weight 0 adds nothing either
  std::vector<int64_t> want = run(gone, true, 20, 20, 1, false).block;
  want.back() = kMlrFlagBadInput;
  auto flagged = [&](const Data<double>& d) { return run(d, true, 20, 20, 4, true).block == want; };
  for (double bad : {-1.0, 0.5, 3.0, nan, inf}) { Data<double> d = base; d.y[row] = bad; EXPECT(flagged(d)); }
  for (double bad : {-2.0, nan, inf}) { Data<double> d = base; d.w[row] = bad; EXPECT(flagged(d)); }
  for (double bad : {nan, inf, -inf}) { Data<double> d = base; d.val[at] = bad; EXPECT(flagged(d)); }
  { Data<double> d = base; d.idx[at] = d.F; EXPECT(flagged(d)); }
  { Data<double> d = base; d.idx[at] = -1; EXPECT(flagged(d)); }
  EXPECT(mlr_weight_ok(0.0) && !mlr_weight_ok(-0.5) && !mlr_weight_ok(nan) && mlr_value_ok(-3.0) && !mlr_value_ok(inf));
}

int main() {
  for (int C : {2, 3, kNbMaxClasses}) {
    test_eval<double>(C);
    test_eval<float>(C);
  }
  test_clamp();
  test_flags();
  if (g_fail) {
    std::fprintf(stderr, "mlr selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("mlr selftest ok\n");
  return 0;
}
