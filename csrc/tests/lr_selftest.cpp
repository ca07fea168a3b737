// Stand-alone self-test of the elastic-net logistic-regression host twins (lr_cpu.cpp) for
// sanitizer builds: rows of 0, 1, 63, 64, 65 and 129 entries with saturated margins, row counts
// around one partial and around the reducer's width, parameter vectors of 1, 2, 255, 256, 257 and
// 65537 slots (buffers sized exactly, so a read or write past the intercept slot is caught), the
// projection to exact zeros, and the sums against the same tree fed with the per-element outputs.
// Built with -fsanitize=address,undefined by
// fraud_detection_spark_kafka_llm_amd/_build.py:build_selftest("lr"); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lr.h"
#include "ops.h"

using namespace fdx;

static int g_fail = 0;
#define EXPECT(c)                                                       \
  do {                                                                  \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double rnd() {      // xorshift64*, uniform in [0, 1)
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static double reduce_ref(const std::vector<double>& terms) {     // lr_reduce over exactly these partials
  double out = 0.0;
  LrReduceArgs a{terms.data(), 1, (int64_t)terms.size(), &out};
  lr_reduce_cpu(a);
  return out;
}

static void test_terms() {
  for (double m : {0.0, 40.0, -40.0, 800.0, -800.0, 1e-300, -1e-300})
    for (double y : {0.0, 1.0}) {
      const LrRowTerms t = lr_row_terms(m, y, 3.0);
      EXPECT(std::isfinite(t.loss) && std::isfinite(t.r) && t.loss >= 0.0);
      EXPECT(std::fabs(t.r) <= 3.0);
    }
  EXPECT(lr_row_terms(0.0, 1.0, 1.0).r == -0.5 && lr_row_terms(800.0, 1.0, 1.0).r == 0.0);
  EXPECT(lr_row_terms(-800.0, 0.0, 2.0).r == 0.0 && lr_row_terms(800.0, 0.0, 1.0).loss == 800.0);
  // projection: leaving the orthant gives +0.0, the intercept is never projected
  LrStepTerms s = lr_step_terms(1.0, -2.0, 1.0, 0.5, 2.0, 1.0, true);
  EXPECT(same_bits(s.x_new, 0.0) && same_bits(s.xs_new, 0.0) && s.dec == -0.5);
  s = lr_step_terms(1.0, -2.0, 0.0, 0.5, 0.0, 1.0, false);
  EXPECT(s.x_new == -1.0 && s.l1 == 0.0 && s.sq == 0.0);
  s = lr_step_terms(0.0, -0.0, -1.0, 0.0, 1.0, 1.0, true);
  EXPECT(same_bits(s.x_new, 0.0));
  // pseudo-gradient at zero: inside the dead zone 0, outside it the nearer one-sided derivative
  EXPECT(lr_grad_terms(0.5, 1.0, 1.0, 0.0, 1.0, 0.0).pg == 0.0 && lr_grad_terms(0.5, 1.0, 1.0, 0.0, 1.0, 0.0).xi == 0.0);
  EXPECT(lr_grad_terms(3.0, 1.0, 1.0, 0.0, 1.0, 0.0).pg == 2.0 && lr_grad_terms(3.0, 1.0, 1.0, 0.0, 1.0, 0.0).xi == -1.0);
  EXPECT(lr_grad_terms(-3.0, 1.0, 1.0, 0.0, 1.0, 0.0).pg == -2.0 && lr_grad_terms(-3.0, 1.0, 1.0, 0.0, 1.0, 0.0).xi == 1.0);
  EXPECT(lr_grad_terms(0.0, 1.0, 1.0, 2.0, 1.0, 0.5).pg == 2.0 && lr_grad_terms(0.0, 1.0, 1.0, -2.0, 1.0, 0.5).pg == -2.0);
}

static void test_forward(int64_t rows, int threads) {
  const int lens[6] = {0, 1, 63, 64, 65, 129};
  const int F = 200;
  std::vector<int64_t> indptr(rows + 1, 0);
  std::vector<int32_t> idx;
  std::vector<float> val;
  for (int64_t r = 0; r < rows; ++r) {
    const int len = lens[r % 6];
    for (int k = 0; k < len; ++k) {
      idx.push_back(k);
      val.push_back((float)(rnd() - 0.5));
    }
    indptr[r + 1] = (int64_t)idx.size();
  }
  std::vector<double> xs(F), y(rows), w(rows);
  for (double& v : xs) v = 4.0 * (rnd() - 0.5);
  const double wv[3] = {0.0, 0.5, 3.0};
  for (int64_t r = 0; r < rows; ++r) y[r] = (r & 1) ? 1.0 : 0.0, w[r] = wv[r % 3];
  const int64_t P = lr_forward_partials(rows);
  for (double b : {0.0, 800.0, -800.0}) {
    std::vector<double> res(rows), loss(rows), margin(rows), partials(2 * P), spmv(rows);
    LrForwardArgs<float> a{indptr.data(), idx.data(), val.data(), rows, xs.data(), &b, y.data(), w.data(),
                           res.data(), loss.data(), margin.data(), partials.data()};
    lr_forward_cpu<float>(a, threads);
    spmv_cpu<float>(indptr.data(), idx.data(), val.data(), xs.data(), spmv.data(), rows, 1);
    std::vector<double> wl(P, 0.0), rs(P, 0.0);
    for (int64_t r = 0; r < rows; ++r) {
      EXPECT(same_bits(margin[r], spmv[r] + b));
      const LrRowTerms t = lr_row_terms(margin[r], y[r], w[r]);
      EXPECT(same_bits(t.r, res[r]) && same_bits(t.loss, loss[r]) && std::isfinite(t.loss) && std::isfinite(t.r));
      wl[r / kLrRowsPerPartial] += w[r] * loss[r];
      rs[r / kLrRowsPerPartial] += res[r];
    }
    for (int64_t p = 0; p < P; ++p) EXPECT(same_bits(wl[p], partials[p]) && same_bits(rs[p], partials[P + p]));
    double out[2];
    LrReduceArgs ra{partials.data(), 2, P, out};
    lr_reduce_cpu(ra);
    EXPECT(same_bits(out[0], reduce_ref(wl)) && same_bits(out[1], reduce_ref(rs)));
    // a null loss_row / margin is allowed
    LrForwardArgs<float> a2 = a;
    a2.loss_row = nullptr;
    a2.margin = nullptr;
    std::vector<double> partials2(2 * P);
    a2.partials = partials2.data();
    lr_forward_cpu<float>(a2, 1);
    EXPECT(partials2 == partials);
  }
}

static void test_params(int64_t n, int threads) {
  const int64_t F = n - 1, G = lr_param_groups(n);
  std::vector<double> x(n), d(n), xi(n), pg(n), scale(F), parts(F + 2);
  for (int64_t j = 0; j < n; ++j) {
    const int kind = (int)(j % 5);
    x[j] = kind == 0 ? 0.0 : 2.0 * (rnd() - 0.5);
    d[j] = kind == 1 ? -4.0 * x[j] : rnd() - 0.5;      // kind 1 flips its sign under a unit step
    pg[j] = kind == 2 ? 0.0 : rnd() - 0.5;
    xi[j] = x[j] > 0 ? 1.0 : (x[j] < 0 ? -1.0 : (pg[j] < 0 ? 1.0 : (pg[j] > 0 ? -1.0 : 0.0)));
  }
  for (int64_t j = 0; j < F; ++j) scale[j] = j % 7 == 3 ? 0.0 : 0.5 + rnd();
  for (double& v : parts) v = 8.0 * (rnd() - 0.5);
  for (double t : {1.0, 0.0078125}) {
    std::vector<double> x_new(n), xs_new(F), partials(3 * G);
    LrStepArgs a{x.data(), d.data(), xi.data(), pg.data(), scale.data(), t, F, x_new.data(), xs_new.data(), partials.data()};
    lr_owlqn_step_cpu(a, threads);
    std::vector<double> l1(G, 0.0), sq(G, 0.0), dec(G, 0.0);
    EXPECT(same_bits(x_new[F], x[F] + t * d[F]));      // the intercept is never projected
    for (int64_t j = 0; j < F; ++j) {
      const double v = x[j] + t * d[j];
      const bool keep = (xi[j] > 0 && v > 0) || (xi[j] < 0 && v < 0);
      EXPECT(same_bits(x_new[j], keep ? v : 0.0) && same_bits(xs_new[j], scale[j] * x_new[j]));
    }
    double out[3];
    LrReduceArgs ra{partials.data(), 3, G, out};
    lr_reduce_cpu(ra);
    double al1 = 0.0, asq = 0.0, adec = 0.0, mag = 0.0;
    for (int64_t j = 0; j < n; ++j) {
      if (j < F) al1 += std::fabs(x_new[j]), asq += x_new[j] * x_new[j];
      adec += pg[j] * (x_new[j] - x[j]);
      mag += std::fabs(pg[j] * (x_new[j] - x[j]));
    }
    const double eps = std::ldexp((double)n, -53);
    EXPECT(std::fabs(out[0] - al1) <= eps * al1 && std::fabs(out[1] - asq) <= eps * asq && std::fabs(out[2] - adec) <= eps * mag);
    // one thread and many threads give the same bits
    std::vector<double> x_new1(n), xs_new1(F), partials1(3 * G);
    LrStepArgs a1 = a;
    a1.x_new = x_new1.data(), a1.xs_new = xs_new1.data(), a1.partials = partials1.data();
    lr_owlqn_step_cpu(a1, 1);
    EXPECT(partials1 == partials && x_new1 == x_new);
  }
  for (bool fit : {true, false}) {
    std::vector<double> g(n), pgo(n), xio(n), partials(G);
    const double W = 37.0, l1 = 0.125, l2 = 0.25;
    LrGradArgs a{parts.data(), scale.data(), x.data(), W, l1, l2, F, fit, g.data(), pgo.data(), xio.data(), partials.data()};
    lr_pseudo_grad_cpu(a, threads);
    EXPECT(same_bits(g[F], fit ? parts[1] / W : 0.0) && same_bits(pgo[F], g[F]) && xio[F] == 0.0);
    double nn = 0.0;
    for (int64_t j = 0; j < n; ++j) {
      if (j < F) {
        const LrGradTerms u = lr_grad_terms(parts[2 + j], scale[j], W, x[j], l1, l2);
        EXPECT(same_bits(u.g, g[j]) && same_bits(u.pg, pgo[j]) && same_bits(u.xi, xio[j]));
        if (x[j] == 0.0) EXPECT(std::fabs(pgo[j]) <= std::fabs(g[j]));
      }
      nn += pgo[j] * pgo[j];
    }
    double out = 0.0;
    LrReduceArgs ra{partials.data(), 1, G, &out};
    lr_reduce_cpu(ra);
    EXPECT(std::fabs(out - nn) <= std::ldexp((double)n, -53) * nn);
  }
}

int main() {
  test_terms();
  for (int64_t rows : {0, 1, 3, 4, 5, 1025, 4099})
    for (int threads : {1, 4}) test_forward(rows, threads);
  for (int64_t n : {1, 2, 255, 256, 257, 65537, 2 * 256 * 1024 + 3})
    for (int threads : {1, 4}) test_params(n, threads);
  if (g_fail) {
    std::fprintf(stderr, "%d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("lr selftest ok\n");
  return 0;
}
