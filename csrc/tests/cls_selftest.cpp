// Stand-alone self-test of the class-score tail of the fused featurizer's host twin (text_cpu.cpp)
// for sanitizer builds: dialogues with 0, 1, 63, 64, 65, 129 and 200 distinct terms and random ones,
// 2, 3 and 8 classes, with and without IDF, unigrams and bigrams, the stored (fp32) and the exact
// (fp64) values, on one and several threads. W, b and the score buffer have exactly the sizes the
// contract names, so a read or write past them is an AddressSanitizer report. The scores are
// compared bit for bit with the lane-order sum taken here over the CSR the same call wrote. Built
// with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("cls"); exits non-zero on failure.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ops.h"
#include "scoring.h"

using namespace fdx;

static int g_fail = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static uint32_t g_rng = 2463534242u;
static uint32_t next_u32() { return g_rng = g_rng * 1664525u + 1013904223u; }
static double next_signed() { return ((double)(next_u32() >> 8) / (double)(1u << 24) - 0.5) * (double)(1 + (next_u32() >> 28)); }

static std::string word(int i) {
  std::string w = "q";
  for (int k = 0; k < 3; ++k) { w.push_back((char)('a' + i % 26)); i /= 26; }
  return w;
}

static std::vector<std::string> documents() {
  std::vector<std::string> docs = {"", " ", "hello there", "Hello, World! hello"};
  for (int k : {0, 1, 63, 64, 65, 129, 200}) {
    std::string d;
    for (int i = 0; i < k; ++i) d += word(i) + " ";
    docs.push_back(d);
  }
  for (int i = 0; i < 120; ++i) {
    std::string d;
    const int T = (int)(next_u32() >> 24) % 90;
    for (int t = 0; t < T; ++t) d += word((int)(next_u32() >> 20) % 150) + ((next_u32() >> 9) % 5 == 0 ? "  " : " ");
    docs.push_back(d);
  }
  return docs;
}

// lane-strided partials of 64 lanes, the xor butterfly (lane 0), then + b_c
static void reference(const int32_t* idx, const double* x, int nu, const double* W, const double* b, int C, double* out) {
  double part[64][kMaxClasses];
  for (auto& p : part) for (double& v : p) v = 0.0;
  for (int j = 0; j < nu; ++j)
    for (int c = 0; c < C; ++c) { const double t = x[j] * W[(int64_t)idx[j] * C + c]; part[j & 63][c] = part[j & 63][c] + t; }
  for (int o = 32; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l)
      for (int c = 0; c < C; ++c) part[l][c] = part[l][c] + part[l ^ o][c];
  for (int c = 0; c < C; ++c) out[c] = part[0][c] + b[c];
}

static void run_mode(const std::vector<std::string>& docs, int C, bool use_idf, int n, bool exact, int threads) {
  std::vector<uint8_t> text;
  std::vector<int64_t> off = {0};
  for (auto& d : docs) { text.insert(text.end(), d.begin(), d.end()); off.push_back((int64_t)text.size()); }
  text.resize(text.size() + 16, 0);
  const int64_t D = (int64_t)docs.size();
  const int F = 4099;
  std::vector<double> idf(F), W((size_t)F * C), b(C);
  for (double& v : idf) v = 0.25 + (double)(next_u32() >> 8) / (double)(1u << 22);
  for (double& v : W) v = next_signed();
  for (double& v : b) v = next_signed();

  const int64_t cap = csr_capacity((int64_t)text.size(), D);
  std::vector<int32_t> idx(cap), nnz(D), ntok(D), status(D, -1), cidx(cap), cnnz(D), cstatus(D, -1);
  std::vector<float> val(cap), cval(cap);
  std::vector<double> raw((size_t)D * C, -1.0), craw(D);
  FeatArgs a{};
  a.text = text.data();
  a.doc_off = off.data();
  a.num_docs = (int32_t)D;
  a.flags = kFlagClean | kFlagWriteCsr | ((n - 1) << kNgramShift);
  a.num_features = F;
  a.stop.mask = -1;
  a.vocab.mask = -1;
  a.min_tf = 1.0;
  a.out_ntok = ntok.data();

  FeatArgs counts = a;               // the term counts, for the exact values
  counts.out_idx = cidx.data();
  counts.out_val = cval.data();
  counts.out_nnz = cnnz.data();
  counts.out_raw = craw.data();
  counts.out_status = cstatus.data();
  featurize_score_cpu(counts, nullptr, 0, threads);

  a.flags |= kFlagClasses | (exact ? kFlagClassExact : 0) | (use_idf ? kFlagIdf : 0);
  a.idf = use_idf ? idf.data() : nullptr;
  a.cls_w = W.data();
  a.cls_b = b.data();
  a.num_classes = C;
  a.out_idx = idx.data();
  a.out_val = val.data();
  a.out_nnz = nnz.data();
  a.out_raw = raw.data();
  a.out_status = status.data();
  featurize_score_cpu(a, nullptr, 0, threads);

  for (int64_t d = 0; d < D; ++d) {
    EXPECT(status[d] == kStatusOk && cstatus[d] == kStatusOk && nnz[d] == cnnz[d]);
    const int64_t base = csr_slot(off[d], d);
    std::vector<double> x(nnz[d]);
    for (int32_t j = 0; j < nnz[d]; ++j) {
      EXPECT(idx[base + j] == cidx[base + j] && idx[base + j] >= 0 && idx[base + j] < F);
      double v = (double)cval[base + j];
      if (use_idf) v = v * idf[idx[base + j]];
      EXPECT(val[base + j] == (float)v);
      x[j] = exact ? v : (double)val[base + j];
    }
    double want[kMaxClasses];
    reference(idx.data() + base, x.data(), nnz[d], W.data(), b.data(), C, want);
    EXPECT(std::memcmp(want, raw.data() + d * C, sizeof(double) * C) == 0);
  }
}

int main() {
  const auto docs = documents();
  for (int C : {2, 3, kMaxClasses})
    for (bool use_idf : {false, true})
      for (int n : {1, 2})
        for (bool exact : {false, true}) run_mode(docs, C, use_idf, n, exact, exact ? 4 : 1);
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("cls selftest ok\n");
  return 0;
}
