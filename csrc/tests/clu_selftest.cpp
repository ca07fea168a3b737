// Stand-alone self-test of the bisecting KMeans and silhouette host twins (clu_cpu.cpp) for sanitizer
// builds: 513 rows (the first of 0, 1, 63, 64, 65 and 130 entries), km_group_step with W = 1 (G = 1,
// 9, 64) and W = 2 (G = 1, 5, 32) and every third row skipped, sil_score with K = 2, 8, 9 and 64, an
// absent and a singleton cluster, fp32 and fp64 values, unit and non-dyadic weights, both measures, 1,
// 2 and 7 threads; every buffer is sized exactly, so a read or write past a row, a cluster or the
// feature space is caught. Both ops are compared with a scalar evaluation of the contract written in
// this file and across the thread counts, assign-only with the full pass; a bad weight, value,
// feature id, group and label must set the flag word and add nothing, and a skipped row with such
// content must set none.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("clu"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "clu.h"

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
constexpr int kK = 30, kKw = 35, kKc = 20, kKs = 33;

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
static Data<V> make(int rows, bool cosine) {
  Data<V> d;
  for (int len : {0, 1, 63, 64, 65, 130}) d.add_row(cosine && len == 0 ? 1 : len);   // no zero row under cosine
  while (d.rows() < rows) d.add_row(1 + (int)(rnd64() % 40));
  return d;
}

static double lane_sum(const std::vector<double>& terms) {
  double p[kNbWave] = {0};
  for (size_t i = 0; i < terms.size(); ++i) p[i & (kNbWave - 1)] += terms[i];
  for (int o = kNbWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) p[l] += p[l + o];
  return p[0];
}

static int64_t quant(double t, int k) { return (int64_t)std::nearbyint(std::ldexp(t, k)); }

// K columns of random values in [F, Kp]; `unit`: columns of norm 1
static std::vector<double> make_columns(int K, bool unit) {
  const int Kp = km_padded(K);
  std::vector<double> CT((size_t)kF * Kp, 0.0);
  for (int j = 0; j < K; ++j) {
    double nn = 0.0;
    for (int f = 0; f < kF; ++f) {
      const double v = rnd() < 0.3 ? 2.0 * rnd() - 0.4 : 0.0;
      CT[(size_t)f * Kp + j] = v;
      nn += v * v;
    }
    if (unit && nn > 0.0)
      for (int f = 0; f < kF; ++f) CT[(size_t)f * Kp + j] /= std::sqrt(nn);
  }
  return CT;
}

static std::vector<double> column_norms(const std::vector<double>& CT, int K) {
  const int Kp = km_padded(K);
  std::vector<double> cn((size_t)Kp, 0.0);
  for (int j = 0; j < K; ++j)
    for (int f = 0; f < kF; ++f) cn[j] += CT[(size_t)f * Kp + j] * CT[(size_t)f * Kp + j];
  return cn;
}

// ---------------------------------------------------------------- km_group_step
struct GroupOut {
  std::vector<int64_t> block;      // [S K F |] Wq K | cnt K | costq K | flag
  std::vector<int32_t> assign;
  std::vector<double> dist;
};

template <class V>
static GroupOut run_group(const Data<V>& d, const std::vector<int32_t>& group, int W, int G, const std::vector<double>& CT,
                          const std::vector<double>& cn, int measure, bool weighted, bool sums, int threads) {
  const int K = clu_centers(W, G);
  GroupOut o;
  o.block.assign((size_t)(sums ? K * kF : 0) + 3 * K + 1, 0);
  o.assign.assign((size_t)d.rows(), 7777);
  o.dist.assign((size_t)d.rows(), -1.0);
  KmGroupArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.labels = nullptr; a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = kF;
  a.slot_of = nullptr; a.hot_feat = nullptr; a.hot_slots = 0; a.chunk_rows = kNbChunkRows;
  a.W = W; a.G = G; a.K = K; a.Kp = km_padded(K); a.measure = measure; a.k = kK; a.kw = kKw; a.kc = kKc;
  a.group = group.data(); a.CT = CT.data(); a.cn = cn.data();
  int64_t* p = o.block.data();
  a.S = sums ? p : nullptr;
  a.Wq = p + (sums ? K * kF : 0); a.cnt = a.Wq + K; a.costq = a.cnt + K; a.flag = a.costq + K;
  a.assign = o.assign.data(); a.dist = o.dist.data();
  km_group_step_cpu<V>(a, threads);
  return o;
}

// the contract, a row at a time (clean input)
template <class V>
static GroupOut direct_group(const Data<V>& d, const std::vector<int32_t>& group, int W, int G,
                             const std::vector<double>& CT, const std::vector<double>& cn, int measure, bool weighted) {
  const int K = clu_centers(W, G), Kp = km_padded(K);
  GroupOut o;
  o.block.assign((size_t)K * kF + 3 * K + 1, 0);
  o.assign.assign((size_t)d.rows(), -1);
  o.dist.assign((size_t)d.rows(), 0.0);
  int64_t* S = o.block.data();
  int64_t *Wq = S + K * kF, *cnt = Wq + K, *costq = cnt + K;
  for (int64_t r = 0; r < d.rows(); ++r) {
    const int g = group[r];
    if (g < 0) continue;
    const double w = weighted ? d.w[r] : 1.0;
    std::vector<double> sq;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) sq.push_back((double)d.val[j] * (double)d.val[j]);
    const double xn = lane_sum(sq), nrm = std::sqrt(xn);
    int best = -1;
    double best_d = 0.0;
    for (int i = 0; i < W; ++i) {
      const int j = W * g + i;
      std::vector<double> t;
      for (int64_t e = d.indptr[r]; e < d.indptr[r + 1]; ++e) t.push_back((double)d.val[e] * CT[(size_t)d.idx[e] * Kp + j]);
      const double dot = lane_sum(t);
      const double dj = measure == kKmCosine ? 1.0 - dot / nrm : std::fmax((xn + cn[j]) - 2.0 * dot, 0.0);
      if (best < 0 || dj < best_d) { best = j; best_d = dj; }
    }
    o.assign[r] = best;
    o.dist[r] = best_d;
    Wq[best] += quant(w, kKw);
    cnt[best] += 1;
    costq[best] += quant(w * best_d, kKc);
    const double s = measure == kKmCosine ? w / nrm : w;
    for (int64_t e = d.indptr[r]; e < d.indptr[r + 1]; ++e) S[(size_t)best * kF + d.idx[e]] += quant(s * (double)d.val[e], kK);
  }
  return o;
}

static std::vector<int32_t> make_groups(int64_t rows, int G) {
  std::vector<int32_t> g((size_t)rows);
  for (int64_t r = 0; r < rows; ++r) g[r] = r % 3 == 1 ? -1 : (int32_t)((r * 7 + 5) % G);
  return g;
}

template <class V>
static void test_group(int W, int G) {
  const int K = clu_centers(W, G);
  for (int measure : {kKmEuclidean, kKmCosine}) {
    const Data<V> d = make<V>(513, measure == kKmCosine);
    const std::vector<double> CT = make_columns(K, measure == kKmCosine), cn = column_norms(CT, K);
    const std::vector<int32_t> group = make_groups(d.rows(), G);
    for (bool weighted : {false, true}) {
      const GroupOut want = direct_group(d, group, W, G, CT, cn, measure, weighted);
      for (int threads : {1, 2, 7}) {
        const GroupOut got = run_group(d, group, W, G, CT, cn, measure, weighted, true, threads);
        EXPECT(same(got.block, want.block) && same(got.assign, want.assign) && same(got.dist, want.dist));
        const GroupOut only = run_group(d, group, W, G, CT, cn, measure, weighted, false, threads);
        EXPECT(same(only.assign, want.assign) && same(only.dist, want.dist));
        EXPECT(std::memcmp(only.block.data(), want.block.data() + (size_t)K * kF, only.block.size() * 8) == 0);
      }
    }
  }
}

static void test_group_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Data<double> base = make<double>(300, true);
  const std::vector<double> CT = make_columns(10, false), cn = column_norms(CT, 10);
  const std::vector<int32_t> group = make_groups(base.rows(), 5);
  // rows 3, 5 and 6 are live (r % 3 != 1), row 4 is skipped
  auto check = [&](const Data<double>& d, const std::vector<int32_t>& g, int measure, int64_t row) {
    const GroupOut got = run_group(d, g, 2, 5, CT, cn, measure, true, true, 2);
    EXPECT(got.block.back() == 1 && got.assign[row] == -1 && got.dist[row] == 0.0);
    std::vector<int32_t> without = group;                 // the flagged row adds nothing
    without[row] = -1;
    GroupOut want = run_group(base, without, 2, 5, CT, cn, measure, true, true, 1);
    EXPECT(want.block.back() == 0);
    want.block.back() = 1;
    EXPECT(same(got.block, want.block));
  };
  for (double bad : {0.0, -2.0, nan, inf}) { Data<double> d = base; d.w[5] = bad; check(d, group, kKmEuclidean, 5); }
  for (double bad : {nan, inf, -inf}) { Data<double> d = base; d.val[(size_t)d.indptr[3]] = bad; check(d, group, kKmEuclidean, 3); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = kF; check(d, group, kKmEuclidean, 3); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = -1; check(d, group, kKmCosine, 3); }
  for (int32_t bad : {5, 1 << 30}) { std::vector<int32_t> g = group; g[6] = bad; check(base, g, kKmEuclidean, 6); }
  { Data<double> d = base; for (int64_t j = d.indptr[6]; j < d.indptr[7]; ++j) d.val[j] = 0.0; check(d, group, kKmCosine, 6); }
  {                                                       // a skipped row is not read
    Data<double> d = base;
    d.w[4] = nan;
    d.idx[(size_t)d.indptr[4]] = 1 << 30;
    d.val[(size_t)d.indptr[4]] = inf;
    const GroupOut got = run_group(d, group, 2, 5, CT, cn, kKmEuclidean, true, true, 2);
    const GroupOut want = run_group(base, group, 2, 5, CT, cn, kKmEuclidean, true, true, 1);
    EXPECT(got.block.back() == 0 && same(got.block, want.block) && same(got.assign, want.assign));
  }
  EXPECT(clu_centers(1, 1) == 2 && clu_centers(2, 1) == 2 && clu_centers(1, 9) == 9 && clu_centers(2, 32) == 64);
}

// ---------------------------------------------------------------- sil_score
struct Stats {
  int K, Kp;
  std::vector<double> MT, psi, nw;
  std::vector<int32_t> cnt;
};

struct SilOut {
  std::vector<int64_t> block;      // silq | wq | flag
  std::vector<double> s;
};

// labels by turns over the clusters c with c % 3 != 2 (those are absent), row 9 alone in a cluster of its own
static std::vector<int32_t> make_labels(int64_t rows, int K, int* single) {
  std::vector<int32_t> present;
  for (int c = 0; c < K; ++c)
    if (K <= 3 || c % 3 != 2) present.push_back(c);
  *single = K > 3 ? present.back() : -1;
  if (K > 3) present.pop_back();
  std::vector<int32_t> lab((size_t)rows);
  for (int64_t r = 0; r < rows; ++r) lab[r] = present[(size_t)((r * 5 + 3) % (int64_t)present.size())];
  if (*single >= 0) lab[9] = *single;
  return lab;
}

template <class V>
static Stats make_stats(const Data<V>& d, const std::vector<int32_t>& lab, int K, int measure, bool weighted) {
  Stats s{K, km_padded(K), {}, {}, {}, {}};
  s.MT.assign((size_t)kF * s.Kp, 0.0);
  s.psi.assign((size_t)s.Kp, 0.0);
  s.nw.assign((size_t)s.Kp, 0.0);
  s.cnt.assign((size_t)s.Kp, 0);
  for (int64_t r = 0; r < d.rows(); ++r) {
    const double w = weighted ? d.w[r] : 1.0;
    double xn = 0.0;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) xn += (double)d.val[j] * (double)d.val[j];
    const double scale = measure == kKmCosine ? w / std::sqrt(xn) : w;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) s.MT[(size_t)d.idx[j] * s.Kp + lab[r]] += scale * (double)d.val[j];
    if (measure != kKmCosine) s.psi[lab[r]] += w * xn;
    s.nw[lab[r]] += w;
    s.cnt[lab[r]] += 1;
  }
  for (int c = 0; c < K; ++c) {
    if (!(s.nw[c] > 0.0)) continue;
    for (int f = 0; f < kF; ++f) s.MT[(size_t)f * s.Kp + c] /= s.nw[c];
    s.psi[c] /= s.nw[c];
  }
  return s;
}

template <class V>
static SilOut run_sil(const Data<V>& d, const std::vector<int32_t>& lab, const Stats& st, int measure, bool weighted,
                      int threads) {
  SilOut o;
  o.block.assign(3, 0);
  o.s.assign((size_t)d.rows(), -7.0);
  SilArgs<V> a{};
  a.indptr = d.indptr.data(); a.idx = d.idx.data(); a.val = d.val.data();
  a.labels = nullptr; a.weights = weighted ? d.w.data() : nullptr;
  a.rows = d.rows(); a.F = kF;
  a.slot_of = nullptr; a.hot_feat = nullptr; a.hot_slots = 0; a.chunk_rows = kNbChunkRows;
  a.K = st.K; a.Kp = st.Kp; a.measure = measure; a.ks = kKs; a.kw = kKw;
  a.label = lab.data(); a.MT = st.MT.data(); a.psi = st.psi.data(); a.nw = st.nw.data(); a.cnt = st.cnt.data();
  a.silq = o.block.data(); a.wq = a.silq + 1; a.flag = a.silq + 2;
  a.s = o.s.data();
  sil_score_cpu<V>(a, threads);
  return o;
}

// the contract, a row and a cluster at a time (clean input)
template <class V>
static SilOut direct_sil(const Data<V>& d, const std::vector<int32_t>& lab, const Stats& st, int measure, bool weighted) {
  SilOut o;
  o.block.assign(3, 0);
  o.s.assign((size_t)d.rows(), 0.0);
  for (int64_t r = 0; r < d.rows(); ++r) {
    const double w = weighted ? d.w[r] : 1.0;
    const int a = lab[r];
    std::vector<double> sq;
    for (int64_t j = d.indptr[r]; j < d.indptr[r + 1]; ++j) sq.push_back((double)d.val[j] * (double)d.val[j]);
    const double xn = lane_sum(sq), nrm = std::sqrt(xn);
    double own_raw = 0.0, nb = 0.0;
    bool have = false;
    for (int c = 0; c < st.K; ++c) {
      std::vector<double> t;
      for (int64_t e = d.indptr[r]; e < d.indptr[r + 1]; ++e) t.push_back((double)d.val[e] * st.MT[(size_t)d.idx[e] * st.Kp + c]);
      const double dot = lane_sum(t);
      const double D = measure == kKmCosine ? 1.0 - dot / nrm : (xn + st.psi[c]) - 2.0 * dot;
      if (c == a) own_raw = D;
      else if (st.nw[c] > 0.0 && (!have || D < nb)) { nb = D; have = true; }
    }
    double s = 0.0;
    if (st.cnt[a] != 1) {
      const double own = (own_raw * st.nw[a]) / (st.nw[a] - w);
      s = own < nb ? 1.0 - own / nb : own > nb ? nb / own - 1.0 : 0.0;
    }
    o.s[r] = s;
    o.block[0] += quant(w * s, kKs);
    o.block[1] += quant(w, kKw);
  }
  return o;
}

template <class V>
static void test_sil(int K) {
  for (int measure : {kKmEuclidean, kKmCosine}) {
    const Data<V> d = make<V>(513, measure == kKmCosine);
    int single;
    const std::vector<int32_t> lab = make_labels(d.rows(), K, &single);
    for (bool weighted : {false, true}) {
      const Stats st = make_stats(d, lab, K, measure, weighted);
      const SilOut want = direct_sil(d, lab, st, measure, weighted);
      if (single >= 0) EXPECT(st.cnt[single] == 1 && want.s[9] == 0.0);
      EXPECT(want.block[0] != 0 && want.block[1] > 0);
      for (int threads : {1, 2, 7}) {
        const SilOut got = run_sil(d, lab, st, measure, weighted, threads);
        EXPECT(same(got.block, want.block) && same(got.s, want.s));
      }
    }
  }
}

static void test_sil_flags() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const Data<double> base = make<double>(300, true);
  int single;
  const std::vector<int32_t> lab = make_labels(base.rows(), 9, &single);
  const Stats st = make_stats(base, lab, 9, kKmEuclidean, true);
  const SilOut clean = run_sil(base, lab, st, kKmEuclidean, true, 1);
  EXPECT(clean.block[2] == 0);
  auto check = [&](const Data<double>& d, const std::vector<int32_t>& l, const Stats& s, int measure, int64_t row) {
    const SilOut got = run_sil(d, l, s, measure, true, 2);
    EXPECT(got.block[2] == 1 && got.s[row] == 0.0);
    if (measure == kKmEuclidean && &s == &st) {           // the flagged row adds nothing: the sums miss its terms
      EXPECT(got.block[0] == clean.block[0] - quant(base.w[row] * clean.s[row], kKs));
      EXPECT(got.block[1] == clean.block[1] - quant(base.w[row], kKw));
    }
  };
  for (double bad : {0.0, -2.0, nan, inf}) { Data<double> d = base; d.w[5] = bad; check(d, lab, st, kKmEuclidean, 5); }
  for (double bad : {nan, inf, -inf}) { Data<double> d = base; d.val[(size_t)d.indptr[3]] = bad; check(d, lab, st, kKmEuclidean, 3); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = kF; check(d, lab, st, kKmEuclidean, 3); }
  { Data<double> d = base; d.idx[(size_t)d.indptr[3] + 2] = -1; check(d, lab, st, kKmEuclidean, 3); }
  for (int32_t bad : {-1, 9, 1 << 30, 2}) { std::vector<int32_t> l = lab; l[6] = bad; check(base, l, st, kKmEuclidean, 6); }   // 2 is absent
  { Data<double> d = base; for (int64_t j = d.indptr[6]; j < d.indptr[7]; ++j) d.val[j] = 0.0; check(d, lab, st, kKmCosine, 6); }
  { Stats s = st; s.nw[lab[7]] = base.w[7] * 0.5; check(base, lab, s, kKmEuclidean, 7); }
  { Stats s = st; s.psi[lab[7]] = inf; check(base, lab, s, kKmEuclidean, 7); }
}

int main() {
  for (int G : {1, 9, 64}) {
    test_group<double>(1, G);
    test_group<float>(1, G);
  }
  for (int G : {1, 5, 32}) {
    test_group<double>(2, G);
    test_group<float>(2, G);
  }
  test_group_flags();
  for (int K : {2, 8, 9, 64}) {
    test_sil<double>(K);
    test_sil<float>(K);
  }
  test_sil_flags();
  if (g_fail) {
    std::fprintf(stderr, "clu_selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("clu_selftest: ok\n");
  return 0;
}
