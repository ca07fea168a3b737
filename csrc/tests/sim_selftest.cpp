// Stand-alone self-test of the top-k cosine retrieval host twins (sim_cpu.cpp) for sanitizer
// builds: corpus rows of 0, 1, 63, 64, 65 and 129 entries, queries of 0, 1, query_cap - 1 and
// query_cap terms stored in ascending and in shuffled order, k of 1, 3 and k_max (also above the
// row count), chunks of 1, 8 and the default number of rows, 1 and 4 threads; every buffer is sized
// exactly, so a read or write past a row, a query or a candidate list is caught. Results are
// compared bit for bit with a direct evaluation of the contract and across the work splits.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("sim"); exits non-zero on failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "sim.h"

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
struct Csr {
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> idx;
  std::vector<V> val;
  int64_t rows() const { return (int64_t)indptr.size() - 1; }
  void add_row(int len, int vocab, bool shuffle) {
    std::vector<int32_t> ids(vocab);
    std::iota(ids.begin(), ids.end(), 0);
    for (int i = 0; i < len; ++i) std::swap(ids[i], ids[i + (int)(rnd64() % (uint64_t)(vocab - i))]);
    if (!shuffle) std::sort(ids.begin(), ids.begin() + len);
    for (int i = 0; i < len; ++i) {
      idx.push_back(ids[i]);
      val.push_back((V)(0.1 + 2.9 * rnd()));
    }
    indptr.push_back((int64_t)idx.size());
  }
};

static double lane_sum(const std::vector<double>& t) {
  double p[kSimWave] = {0};
  for (size_t j = 0; j < t.size(); ++j) p[j & (kSimWave - 1)] += t[j];
  return sim_butterfly_host(p);
}

template <class V>
static std::vector<double> norms_of(const Csr<V>& c) {
  std::vector<double> out(c.rows());
  SimNormArgs<V> a{c.indptr.data(), c.val.data(), c.rows(), out.data()};
  sim_norms_cpu<V>(a, 1);
  for (int64_t r = 0; r < c.rows(); ++r) {
    std::vector<double> t;
    for (int64_t j = c.indptr[r]; j < c.indptr[r + 1]; ++j) t.push_back((double)c.val[j] * (double)c.val[j]);
    EXPECT(same_bits(out[r], std::sqrt(lane_sum(t))));
  }
  return out;
}

struct Result {
  std::vector<int64_t> rows;
  std::vector<double> sims;
};

template <class V>
static Result run(const Csr<V>& c, const std::vector<double>& norms, const Csr<double>& q,
                  const std::vector<double>& qn, int k, int chunk_rows, int threads) {
  const int64_t N = c.rows(), Q = q.rows(), chunks = sim_chunks(N, chunk_rows);
  const int k_out = (int)std::min<int64_t>(k, N);
  std::vector<double> cs((size_t)(Q * chunks * k));
  std::vector<int64_t> cr((size_t)(Q * chunks * k));
  Result res{std::vector<int64_t>((size_t)(Q * k_out)), std::vector<double>((size_t)(Q * k_out))};
  SimTopkArgs<V> a{};
  a.indptr = c.indptr.data(); a.idx = c.idx.data(); a.val = c.val.data(); a.norms = norms.data(); a.rows = N;
  a.q_indptr = q.indptr.data(); a.q_idx = q.idx.data(); a.q_val = q.val.data(); a.q_norms = qn.data(); a.queries = Q;
  a.k = k; a.chunk_rows = chunk_rows; a.queries_per_pass = kSimQueriesPerPass; a.chunks = chunks;
  a.cand_sims = cs.data(); a.cand_rows = cr.data();
  sim_topk_cpu<V>(a, threads);
  SimMergeArgs m{cs.data(), cr.data(), Q, chunks * k, k, k_out, res.sims.data(), res.rows.data()};
  sim_merge_cpu(m, threads);
  return res;
}

template <class V>
static Result direct(const Csr<V>& c, const std::vector<double>& norms, const Csr<double>& q,
                     const std::vector<double>& qn, int k) {
  const int64_t N = c.rows(), Q = q.rows();
  const int k_out = (int)std::min<int64_t>(k, N);
  Result res;
  for (int64_t qq = 0; qq < Q; ++qq) {
    std::vector<double> sim(N);
    for (int64_t r = 0; r < N; ++r) {
      std::vector<double> t;
      for (int64_t j = c.indptr[r]; j < c.indptr[r + 1]; ++j) {
        double x = 0.0;
        for (int64_t i = q.indptr[qq]; i < q.indptr[qq + 1]; ++i)
          if (q.idx[i] == c.idx[j]) x = q.val[i];
        t.push_back((double)c.val[j] * x);
      }
      sim[r] = sim_value(lane_sum(t), norms[r], qn[qq]);
    }
    std::vector<int64_t> order(N);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return sim_better(sim[x], x, sim[y], y); });
    for (int i = 0; i < k_out; ++i) {
      res.rows.push_back(order[i]);
      res.sims.push_back(sim[order[i]]);
    }
  }
  return res;
}

static bool equal(const Result& a, const Result& b) {
  if (a.rows != b.rows || a.sims.size() != b.sims.size()) return false;
  for (size_t i = 0; i < a.sims.size(); ++i)
    if (!same_bits(a.sims[i], b.sims[i])) return false;
  return true;
}

template <class V>
static void test_corpus(int extra_rows) {
  const int vocab = kSimQueryCap + 64;
  Csr<V> c;
  for (int len : {0, 1, 63, 64, 65, 129, 0, 17}) c.add_row(len, vocab, false);
  for (int i = 0; i < extra_rows; ++i) c.add_row((int)(rnd64() % 40), vocab, false);
  c.add_row(17, vocab, false);
  // two identical rows far apart: ties resolve to the smaller row
  const int64_t last = c.rows() - 1;
  for (int64_t j = 0; j < 17; ++j) {
    c.idx[c.indptr[last] + j] = c.idx[c.indptr[7] + j];
    c.val[c.indptr[last] + j] = c.val[c.indptr[7] + j];
  }
  const std::vector<double> norms = norms_of(c);
  for (bool shuffle : {false, true}) {
    Csr<double> q;
    for (int len : {0, 1, 40, kSimQueryCap - 1, kSimQueryCap}) q.add_row(len, vocab, shuffle);
    q.add_row(17, vocab, false);     // the twin rows' own vector
    for (int64_t j = 0; j < 17; ++j) {
      q.idx[q.indptr[5] + j] = c.idx[c.indptr[7] + j];
      q.val[q.indptr[5] + j] = (double)c.val[c.indptr[7] + j];
    }
    const std::vector<double> qn = norms_of(q);
    const Result full = direct(c, norms, q, qn, kSimKMax);
    const int k_full = (int)std::min<int64_t>(kSimKMax, c.rows());
    for (int k : {1, 3, kSimKMax}) {
      const int k_out = (int)std::min<int64_t>(k, c.rows());
      Result want;                              // a smaller k is a prefix of the ranking
      for (int64_t qq = 0; qq < q.rows(); ++qq)
        for (int i = 0; i < k_out; ++i) {
          want.rows.push_back(full.rows[qq * k_full + i]);
          want.sims.push_back(full.sims[qq * k_full + i]);
        }
      if (k_out >= 2) EXPECT(want.rows[5 * k_out] == 7 && want.rows[5 * k_out + 1] == last);
      EXPECT(want.rows[0] == 0 && same_bits(want.sims[0], 0.0));       // the empty query: rows 0 .. k - 1, sim 0.0
      for (int chunk_rows : {1, 8, kSimChunkRows})
        for (int threads : {1, 4}) EXPECT(equal(run(c, norms, q, qn, k, chunk_rows, threads), want));
    }
  }
}

int main() {
  EXPECT(sim_value(1.0, 0.0, 0.0) == 1e12 && same_bits(sim_value(0.0, 0.0, 3.0), 0.0));
  EXPECT(sim_better(1.0, 5, 0.5, 1) && sim_better(0.0, 1, -0.0, 2) && !sim_better(-0.0, 2, 0.0, 1));
  test_corpus<double>(0);                       // fewer rows than k_max
  test_corpus<float>(kSimChunkRows + 3);        // more than one default chunk
  test_corpus<double>(2 * kSimChunkRows);
  if (g_fail) {
    std::fprintf(stderr, "sim_selftest: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("sim_selftest: ok\n");
  return 0;
}
