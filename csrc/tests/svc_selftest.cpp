// Stand-alone self-test of the linear SVC host twin (svc_cpu.cpp) for sanitizer builds: rows of 0,
// 1, 63, 64, 65 and 129 entries, fp32 and fp64 values, unit weights and weights from {0, 0.5, 3},
// negative values, forced margins of exactly +-1, of +-800 and of 5000, and 1 and 3 threads; every
// buffer is sized exactly, so a read or write past a row or the feature space is caught. Margins
// are compared bit for bit with spmv's 64-partial order written out here, the block with a direct
// integer evaluation of the contract and across the thread counts; bad labels, weights, values and
// feature ids must set the high half of the flag word and add nothing, and no value that is not
// finite may reach a conversion to an integer.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("svc"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "svc.h"

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

constexpr int kForced = 5;                         // features 0 .. 4 carry the forced margins
static const double kForcedXs[kForced] = {1.0, -1.0, 800.0, -800.0, 5000.0};

template <class V>
struct Data {
  int F = 300;
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  std::vector<double> y, w, xs;
  double b = 0.0;
  int64_t rows() const { return (int64_t)y.size(); }
  void add_row(int len, double label, double weight) {
    std::vector<int32_t> ids(F - kForced);
    std::iota(ids.begin(), ids.end(), kForced);
    for (int i = 0; i < len; ++i) std::swap(ids[i], ids[i + (int)(rnd64() % (uint64_t)(F - kForced - i))]);
    for (int i = 0; i < len; ++i) {
      idx.push_back(ids[i]);
      val.push_back((V)((rnd() < 0.15 ? -1.0 : 1.0) * (0.1 + 2.9 * rnd())));
    }
    indptr.push_back((int64_t)idx.size());
    y.push_back(label);
    w.push_back(weight);
  }
  void add_forced(int feature, double label, double weight) {
    idx.push_back(feature);
    val.push_back((V)1);
    indptr.push_back((int64_t)idx.size());
    y.push_back(label);
    w.push_back(weight);
  }
};

constexpr int kHead = 8;                           // rows in front of the forced ones

template <class V>
static Data<V> make(int extra_rows, bool with_5000, double b) {
  Data<V> d;
  d.b = b;
  auto label = [&] { return (double)(rnd64() & 1); };
  auto weight = [&] { const double u = rnd(); return u < 0.1 ? 0.0 : u < 0.55 ? 0.5 : 3.0; };
  for (int len : {0, 1, 63, 64, 65, 129, 0, 17}) d.add_row(len, label(), weight());
  // margins of exactly +1 and -1 with both labels, +-800 with the label they agree with, 5000 against label 0
  for (int f = 0; f < 2; ++f)
    for (double y : {0.0, 1.0}) d.add_forced(f, y, 3.0);
  d.add_forced(2, 1.0, 0.5);
  d.add_forced(3, 0.0, 0.5);
  if (with_5000) d.add_forced(4, 0.0, 3.0);
  for (int i = 0; i < extra_rows; ++i) d.add_row((int)(rnd64() % 40), label(), weight());
  d.xs.resize((size_t)d.F);
  for (double& x : d.xs) x = 0.8 * rnd() - 0.4;
  for (int f = 0; f < kForced; ++f) d.xs[f] = kForcedXs[f] - b;   // b is dyadic: exact
  return d;
}

struct Out {
  std::vector<int64_t> block;
  std::vector<double> margin, r, loss;
};

template <class V>
static Out run(const Data<V>& d, bool weighted, int k, int kl, int threads, bool rows) {
  Out o;
  o.block.assign((size_t)d.F + 4, 0);
  if (rows) {
    o.margin.assign((size_t)d.rows(), -7.0);
    o.r.assign((size_t)d.rows(), -7.0);
    o.loss.assign((size_t)d.rows(), -7.0);
  }
  SvcArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.xs = d.xs.data(); a.b = d.b;
  a.labels = d.y.data(); a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = d.F; a.k = k; a.kl = kl;
  a.Gq = o.block.data(); a.gbq = a.Gq + d.F; a.lossq = a.gbq + 1; a.nact = a.lossq + 1; a.flag = a.nact + 1;
  a.margin = rows ? o.margin.data() : nullptr;
  a.r = rows ? o.r.data() : nullptr;
  a.loss_row = rows ? o.loss.data() : nullptr;
  svc_eval_cpu<V>(a, threads);
  return o;
}

// spmv's order written out: lane l adds the entries l, l + 64, ..., then the halving adds, then + b
template <class V>
static double margin_of(const Data<V>& d, int64_t r) {
  double p[64] = {};
  for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j)
    p[(j - d.indptr[r]) % 64] += (double)d.val[j] * d.xs[d.idx[j]];
  for (int o = 32; o > 0; o /= 2)
    for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
  return p[0] + d.b;
}

// the block by the contract, from margins computed here
template <class V>
static std::vector<int64_t> direct(const Data<V>& d, bool weighted, int k, int kl) {
  std::vector<int64_t> out((size_t)d.F + 4, 0);
  for (int64_t r = 0; r < d.rows(); ++r) {
    const double w = weighted ? d.w[r] : 1.0, s = 2.0 * d.y[r] - 1.0;
    const double z = 1.0 - s * margin_of(d, r);
    const bool clamped = !(z < 2048.0);
    const double loss = clamped ? 2048.0 : (z > 0.0 ? z : 0.0);
    const double res = z > 0.0 ? -s * w : 0.0;
    if (clamped) out[d.F + 3] |= kMlrFlagClamped;
    out[d.F + 1] += (int64_t)std::nearbyint(std::ldexp(w * loss, kl));
    if (res == 0.0) continue;
    out[d.F] += (int64_t)std::nearbyint(std::ldexp(res, k));
    out[d.F + 2] += 1;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j)
      out[d.idx[j]] += (int64_t)std::nearbyint(std::ldexp((double)d.val[j] * res, k));
  }
  return out;
}

template <class V>
static void test_eval() {
  const Data<V> d = make<V>(2100, false, 0.25);
  for (bool weighted : {false, true}) {
    const int k = 38, kl = 36;
    const Out ref = run(d, weighted, k, kl, 1, true);
    EXPECT(ref.block.back() == 0);
    EXPECT(ref.block == direct(d, weighted, k, kl));
    EXPECT(run(d, weighted, k, kl, 3, false).block == ref.block);
    const Out again = run(d, weighted, k, kl, 3, true);
    EXPECT(again.block == ref.block && again.r == ref.r && again.loss == ref.loss && again.margin == ref.margin);
    int64_t active = 0;
    for (int64_t r = 0; r < d.rows(); ++r) {
      const double m = margin_of(d, r), w = weighted ? d.w[r] : 1.0;
      EXPECT(std::memcmp(&m, &ref.margin[r], sizeof m) == 0);
      EXPECT(std::fabs(ref.r[r]) == 0.0 || std::fabs(ref.r[r]) == w);
      EXPECT(ref.loss[r] >= 0.0 && ref.loss[r] < kMlrLossCap);
      active += ref.r[r] != 0.0;
    }
    EXPECT(ref.block[d.F + 2] == active);
    // forced rows: (m = +1, y = 0) active, (+1, 1) exactly on the margin and inactive, (-1, 0) inactive,
    // (-1, 1) active, +-800 with the agreeing label inactive
    const double wf = weighted ? 3.0 : 1.0;
    EXPECT(ref.margin[kHead] == 1.0 && ref.r[kHead] == wf && ref.loss[kHead] == 2.0);
    EXPECT(ref.margin[kHead + 1] == 1.0 && ref.r[kHead + 1] == 0.0 && ref.loss[kHead + 1] == 0.0);
    EXPECT(ref.margin[kHead + 2] == -1.0 && ref.r[kHead + 2] == 0.0 && ref.loss[kHead + 2] == 0.0);
    EXPECT(ref.margin[kHead + 3] == -1.0 && ref.r[kHead + 3] == -wf && ref.loss[kHead + 3] == 2.0);
    EXPECT(ref.r[kHead + 4] == 0.0 && ref.r[kHead + 5] == 0.0);
  }
}

static void test_clamp() {
  const double inf = std::numeric_limits<double>::infinity();
  Data<double> d = make<double>(40, true, 0.0);
  const int64_t row = kHead + 6;                  // margin 5000, label 0: z = 5001
  Out o = run(d, true, 30, 28, 3, true);
  EXPECT(o.block.back() == kMlrFlagClamped);
  EXPECT(o.loss[row] == kMlrLossCap && o.r[row] == d.w[row]);
  EXPECT(o.block == direct(d, true, 30, 28));
  for (double bad : {inf, -inf, std::numeric_limits<double>::quiet_NaN()}) {
    Data<double> e = d;
    e.xs[4] = bad;
    const Out p = run(e, true, 30, 28, 1, true);
    EXPECT(p.block.back() == kMlrFlagClamped || bad == -inf);
    if (bad == -inf) {                             // a margin of -inf agrees with label 0: inactive, not clamped
      EXPECT(p.block.back() == 0 && p.loss[row] == 0.0 && p.r[row] == 0.0);
    } else if (bad == inf) {
      EXPECT(p.loss[row] == kMlrLossCap && p.r[row] == d.w[row]);
    } else {
      EXPECT(p.loss[row] == kMlrLossCap && p.r[row] == 0.0);
    }
  }
}

static void test_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Data<double> base = make<double>(900, false, -0.5);
  int64_t row = 20;
  while (base.indptr[row + 1] == base.indptr[row]) ++row;
  const int64_t at = base.indptr[row];
  base.w[row] = 3.0;
  EXPECT(run(base, true, 20, 20, 1, false).block.back() == 0);
  Data<double> gone = base;
  gone.w[row] = 0.0;                             // a row of weight 0 adds nothing either
  std::vector<int64_t> want = run(gone, true, 20, 20, 1, false).block;
  want.back() = kMlrFlagBadInput;
  auto flagged = [&](const Data<double>& d) {
    return run(d, true, 20, 20, 3, true).block == want && run(d, true, 20, 20, 1, false).block == want;
  };
  for (double bad : {-1.0, 0.5, 2.0, nan, inf}) { Data<double> d = base; d.y[row] = bad; EXPECT(flagged(d)); }
  for (double bad : {-2.0, nan, inf}) { Data<double> d = base; d.w[row] = bad; EXPECT(flagged(d)); }
  for (double bad : {nan, inf, -inf}) { Data<double> d = base; d.val[at] = bad; EXPECT(flagged(d)); }
  { Data<double> d = base; d.idx[at] = d.F; EXPECT(flagged(d)); }
  { Data<double> d = base; d.idx[at] = -1; EXPECT(flagged(d)); }
  EXPECT(svc_label_ok(0.0) && svc_label_ok(1.0) && !svc_label_ok(0.5) && !svc_label_ok(nan));
}

// the shared host pass (fixedpoint.h) at 2 * 256 + 1 rows: whatever the thread count asked for, the
// private blocks merge to the single-thread block
static void test_host_merge() {
  const Data<double> d = make<double>(2 * 256 + 1 - kHead - 6, false, 0.25);
  EXPECT(d.rows() == 2 * 256 + 1);
  const Out ref = run(d, true, 38, 36, 1, true);
  EXPECT(ref.block.back() == 0 && ref.block == direct(d, true, 38, 36));
  for (int threads : {1, 2, 7}) {
    const Out o = run(d, true, 38, 36, threads, true);
    EXPECT(o.block == ref.block && o.r == ref.r && o.loss == ref.loss && o.margin == ref.margin);
  }
}

static void test_empty() {
  Data<double> d;
  d.xs.assign((size_t)d.F, 0.0);
  const Out none = run(d, false, 20, 20, 3, true);  // no rows at all
  EXPECT(none.block == std::vector<int64_t>((size_t)d.F + 4, 0));
  for (int i = 0; i < 5; ++i) d.add_row(0, (double)(i & 1), 1.0);
  const Out o = run(d, false, 20, 20, 3, true);     // empty rows at beta = 0: all active, loss 1 each
  EXPECT(o.block[d.F] == (int64_t)(3 - 2) * (int64_t(1) << 20));
  EXPECT(o.block[d.F + 1] == 5 * (int64_t(1) << 20) && o.block[d.F + 2] == 5 && o.block[d.F + 3] == 0);
}

int main() {
  test_eval<double>();
  test_eval<float>();
  test_clamp();
  test_flags();
  test_host_merge();
  test_empty();
  if (g_fail) {
    std::fprintf(stderr, "svc selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("svc selftest ok\n");
  return 0;
}
