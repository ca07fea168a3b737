// Stand-alone self-test of the KMeans host twins (km_cpu.cpp) for sanitizer builds: 513 rows (the
// first of 0, 1, 63, 64, 65 and 130 entries), K = 8 and 9 (the tile boundary) with one center that
// repeats another (it wins no tie), fp32 and fp64 values, unit and non-dyadic weights, both measures, 1, 2 and 7
// threads; every buffer is sized exactly, so a read or write past a row, a cluster or the feature
// space is caught. km_step is compared with a scalar evaluation of the contract written in this
// file and across the thread counts, assign-only with the full pass, km_centers with a scalar
// reference of its summation order; a bad weight, value, feature id and a zero row under cosine
// must set the flag word, add nothing and be assigned -1.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("km"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "km.h"

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

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

constexpr int kF = 300;

template <class V>
struct Data {
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  std::vector<double> w;
  int64_t rows() const { return (int64_t)w.size(); }
  void add_row(int len) {
    std::vector<int32_t> ids(kF);
    std::iota(ids.begin(), ids.end(), 0);
    for (int i = 0; i < len; ++i) std::swap(ids[i], ids[i + (int)(rnd64() % (uint64_t)(kF - i))]);
    for (int i = 0; i < len; ++i) {
      idx.push_back(ids[i]);
      val.push_back((V)(rnd() < 0.2 ? -(0.1 + rnd()) : 0.1 + 2.9 * rnd()));
    }
    indptr.push_back((int64_t)idx.size());
    w.push_back(0.3 + 1.7 * rnd());
  }
};

template <class V>
static Data<V> make(int rows) {
  Data<V> d;
  for (int len : {0, 1, 63, 64, 65, 130}) d.add_row(len);
  while (d.rows() < rows) d.add_row(1 + (int)(rnd64() % 40));
  return d;
}

struct Centers {
  int K, Kp;
  std::vector<double> CT, cn;      // [kF, Kp], [Kp]
};

// K random centers; center `far` > 0 repeats center 0: the smaller index wins every tie, so its cluster stays empty
static Centers make_centers(int K, int far, bool unit) {
  Centers c{K, km_padded(K), {}, {}};
  c.CT.assign((size_t)kF * c.Kp, 0.0);
  c.cn.assign((size_t)c.Kp, 0.0);
  for (int j = 0; j < K; ++j) {
    double nn = 0.0;
    for (int f = 0; f < kF; ++f) {
      const double v = j == far ? c.CT[(size_t)f * c.Kp] : 2.0 * rnd();
      c.CT[(size_t)f * c.Kp + j] = v;
      nn += v * v;
    }
    if (unit && j != far)
      for (int f = 0; f < kF; ++f) c.CT[(size_t)f * c.Kp + j] /= std::sqrt(nn);
    nn = 0.0;
    for (int f = 0; f < kF; ++f) nn += c.CT[(size_t)f * c.Kp + j] * c.CT[(size_t)f * c.Kp + j];
    c.cn[j] = nn;
  }
  return c;
}

struct Out {
  std::vector<int64_t> block;      // [S K F |] Wq K | cnt K | costq | flag
  std::vector<int32_t> assign;
  std::vector<double> dist;
};

template <class V>
static Out run_step(const Data<V>& d, const Centers& c, int measure, bool weighted, bool sums, int threads) {
  const int K = c.K;
  Out o;
  o.block.assign((size_t)(sums ? K * kF : 0) + 2 * K + 2, 0);
  o.assign.assign((size_t)d.rows(), 7777);
  o.dist.assign((size_t)d.rows(), -1.0);
  KmStepArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.labels = nullptr; a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = kF;
  a.slot_of = nullptr; a.hot_feat = nullptr; a.hot_slots = 0; a.chunk_rows = kNbChunkRows;
  a.K = K; a.Kp = c.Kp; a.measure = measure; a.k = 30; a.kw = 35; a.kc = 20;
  a.CT = c.CT.data(); a.cn = c.cn.data();
  int64_t* p = o.block.data();
  a.S = sums ? p : nullptr;
  a.Wq = p + (sums ? K * kF : 0); a.cnt = a.Wq + K; a.costq = a.cnt + K; a.flag = a.costq + 1;
  a.assign = o.assign.data(); a.dist = o.dist.data();
  km_step_cpu<V>(a, threads);
  return o;
}

static double lane_sum(const std::vector<double>& terms) {
  double p[kNbWave] = {0};
  for (size_t i = 0; i < terms.size(); ++i) p[i & (kNbWave - 1)] += terms[i];
  for (int o = kNbWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) p[l] += p[l + o];
  return p[0];
}

// the contract, a row and a center at a time
template <class V>
static Out direct_step(const Data<V>& d, const Centers& c, int measure, bool weighted) {
  const int K = c.K;
  Out o;
  o.block.assign((size_t)K * kF + 2 * K + 2, 0);
  o.assign.assign((size_t)d.rows(), 7777);
  o.dist.assign((size_t)d.rows(), -1.0);
  int64_t* S = o.block.data();
  int64_t *Wq = S + K * kF, *cnt = Wq + K, *costq = cnt + K;
  for (int64_t r = 0; r < d.rows(); ++r) {
    const double w = weighted ? d.w[r] : 1.0;
    std::vector<double> sq;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) sq.push_back((double)d.val[j] * (double)d.val[j]);
    const double xn = lane_sum(sq), nrm = std::sqrt(xn);
    int best = -1;
    double best_d = 0.0;
    for (int j = 0; j < K; ++j) {
      std::vector<double> t;
      for (int64_t e = d.indptr[r]; e < d.indptr[r + 1]; ++e)
        t.push_back((double)d.val[e] * c.CT[(size_t)d.idx[e] * c.Kp + j]);
      const double dot = lane_sum(t);
      const double dj = measure == kKmCosine ? 1.0 - dot / nrm : std::fmax((xn + c.cn[j]) - 2.0 * dot, 0.0);
      if (best < 0 || dj < best_d) { best = j; best_d = dj; }
    }
    o.assign[r] = best;
    o.dist[r] = best_d;
    Wq[best] += (int64_t)std::nearbyint(std::ldexp(w, 35));
    cnt[best] += 1;
    *costq += (int64_t)std::nearbyint(std::ldexp(w * best_d, 20));
    const double s = measure == kKmCosine ? w / nrm : w;
    for (int64_t e = d.indptr[r]; e < d.indptr[r + 1]; ++e)
      S[(size_t)best * kF + d.idx[e]] += (int64_t)std::nearbyint(std::ldexp(s * (double)d.val[e], 30));
  }
  return o;
}

struct NewCenters {
  std::vector<double> CT, cn, moved2;
};

static NewCenters run_centers(const Out& o, const Centers& c, int measure, int threads) {
  const int K = c.K;
  NewCenters n{std::vector<double>((size_t)kF * c.Kp, 0.0), std::vector<double>((size_t)c.Kp, 0.0),
               std::vector<double>((size_t)K, -1.0)};
  KmCentersArgs a{K, c.Kp, kF, measure, 30, 35, o.block.data(), o.block.data() + K * kF, c.CT.data(), n.CT.data(),
                  n.cn.data(), n.moved2.data()};
  km_centers_cpu(a, threads);
  return n;
}

static double strided_sum(const std::vector<double>& v) {      // lane t adds t, t + 256, ..., then the tree
  double s[kKmCentersBlock] = {0};
  for (int t = 0; t < kKmCentersBlock; ++t)
    for (size_t f = (size_t)t; f < v.size(); f += kKmCentersBlock) s[t] += v[f];
  for (int o = kKmCentersBlock / 2; o > 0; o >>= 1)
    for (int t = 0; t < o; ++t) s[t] += s[t + o];
  return s[0];
}

static NewCenters direct_centers(const Out& o, const Centers& c, int measure) {
  const int K = c.K;
  NewCenters n{std::vector<double>((size_t)kF * c.Kp, 0.0), std::vector<double>((size_t)c.Kp, 0.0),
               std::vector<double>((size_t)K, -1.0)};
  const int64_t* S = o.block.data();
  const int64_t* Wq = S + K * kF;
  for (int j = 0; j < K; ++j) {
    std::vector<double> v((size_t)kF), sq((size_t)kF), mv((size_t)kF);
    for (int f = 0; f < kF; ++f) v[f] = c.CT[(size_t)f * c.Kp + j];
    if (Wq[j] != 0) {
      const double W = std::ldexp((double)Wq[j], -35);
      for (int f = 0; f < kF; ++f) v[f] = std::ldexp((double)S[(size_t)j * kF + f], -30) / W;
      if (measure == kKmCosine) {
        for (int f = 0; f < kF; ++f) sq[f] = v[f] * v[f];
        const double nrm = std::sqrt(strided_sum(sq));
        for (int f = 0; f < kF; ++f) v[f] = v[f] / nrm;
      }
    }
    for (int f = 0; f < kF; ++f) {
      n.CT[(size_t)f * c.Kp + j] = v[f];
      sq[f] = v[f] * v[f];
      const double dlt = v[f] - c.CT[(size_t)f * c.Kp + j];
      mv[f] = dlt * dlt;
    }
    n.cn[j] = strided_sum(sq);
    n.moved2[j] = strided_sum(mv);
  }
  return n;
}

template <class V>
static void test_step(int K) {
  const Data<V> d = make<V>(513);
  for (int measure : {kKmEuclidean, kKmCosine}) {
    const int far = K - 1;
    const Centers c = make_centers(K, far, measure == kKmCosine);
    for (bool weighted : {false, true}) {
      Data<V> dd = d;
      if (measure == kKmCosine) {                  // no zero row under cosine: the empty row gets an entry
        dd = Data<V>();
        for (int len : {1, 1, 63, 64, 65, 130}) dd.add_row(len);
        while (dd.rows() < 513) dd.add_row(1 + (int)(rnd64() % 40));
      }
      const Out want = direct_step(dd, c, measure, weighted);
      EXPECT(want.block.back() == 0);
      EXPECT(want.block[(size_t)K * kF + K + far] == 0);            // the far center's cluster is empty
      for (int threads : {1, 2, 7}) {
        const Out got = run_step(dd, c, measure, weighted, true, threads);
        EXPECT(same(got.block, want.block) && same(got.assign, want.assign) && same(got.dist, want.dist));
        const Out only = run_step(dd, c, measure, weighted, false, threads);
        EXPECT(same(only.assign, want.assign) && same(only.dist, want.dist));
        EXPECT(std::memcmp(only.block.data(), want.block.data() + (size_t)K * kF, only.block.size() * 8) == 0);
      }
      const NewCenters ref = direct_centers(want, c, measure);
      for (int threads : {1, 7}) {
        const NewCenters got = run_centers(want, c, measure, threads);
        EXPECT(same(got.CT, ref.CT) && same(got.cn, ref.cn) && same(got.moved2, ref.moved2));
      }
      EXPECT(ref.moved2[far] == 0.0);                                // an empty cluster keeps its center
      for (int f = 0; f < kF; ++f) EXPECT(ref.CT[(size_t)f * c.Kp + far] == c.CT[(size_t)f * c.Kp + far]);
    }
  }
}

static void test_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Data<double> base = make<double>(300);
  const Centers c = make_centers(9, 8, false);
  const Out clean = run_step(base, c, kKmEuclidean, true, true, 1);
  EXPECT(clean.block.back() == 0 && clean.assign[0] >= 0);
  auto check = [&](const Data<double>& d, int measure, int64_t row) {
    const Out got = run_step(d, c, measure, true, true, 2);
    EXPECT(got.block.back() == 1 && got.assign[row] == -1);
    // the flagged row adds nothing: the sums are those of the data without it
    Data<double> rest;
    for (int64_t r = 0; r < d.rows(); ++r) {
      if (r == row) continue;
      for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) { rest.idx.push_back(d.idx[j]); rest.val.push_back(d.val[j]); }
      rest.indptr.push_back((int64_t)rest.idx.size());
      rest.w.push_back(d.w[r]);
    }
    Out want = run_step(rest, c, measure, true, true, 1);
    EXPECT(want.block.back() == 0);
    want.block.back() = 1;
    EXPECT(same(got.block, want.block));
  };
  for (double bad : {0.0, -2.0, nan, inf}) { Data<double> d = base; d.w[5] = bad; check(d, kKmEuclidean, 5); }
  for (double bad : {nan, inf, -inf}) { Data<double> d = base; d.val[(size_t)d.indptr[4]] = bad; check(d, kKmEuclidean, 4); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = kF; check(d, kKmEuclidean, 3); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = -1; check(d, kKmEuclidean, 3); }
  check(base, kKmCosine, 0);                      // row 0 is empty: a zero row under cosine
  EXPECT(km_padded(8) == 8 && km_padded(9) == 16 && km_padded(64) == 64 && km_padded(2) == 8);
}

int main() {
  for (int K : {8, 9}) {
    test_step<double>(K);
    test_step<float>(K);
  }
  test_flags();
  if (g_fail) {
    std::fprintf(stderr, "km_selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("km_selftest: ok\n");
  return 0;
}
