// Multi-class gradient boosting (multi:softprob): the descriptors and the row-term function shared
// by softprob_kernels.hip and softprob_cpu.cpp, so both sides execute the same operations (fp
// contraction is off in both). Two ops:
//   softprob_grad      the round's 2 C gradient planes from the round-start margins. Margins are C
//                      planes M[c][r] (fp64), labels integers 0 .. C - 1 held as fp32, weights fp32 or
//                      absent (1.0); G[c][r], H[c][r] are fp32 planes, what grow_tree takes per class
//   score_class_trees  raw[r, c] = sum of the leaf values of the trees of class c, for a tree list
//                      that carries one int32 class id per tree (any assignment). Lane l of 64 walks
//                      trees l, l + 64, ... ascending and adds each leaf value into its partial of
//                      that tree's class; the C partials meet in the xor butterfly (offsets 32 .. 1)
//                      and lane 0 writes the row. A partial starts at +0.0 and the other classes get
//                      + 0.0, which never changes a bit of them (a sum that starts at +0.0 cannot
//                      become -0.0), so select-and-add equals skipping.
// The class count is a template parameter in both, so the C values of a row stay in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "scoring.h"

#pragma clang fp contract(off)

namespace fdx {

constexpr int kSoftprobMaxClasses = kMaxClasses;
constexpr int kSoftprobWave = 64;
constexpr int kSoftprobBlock = 256;
constexpr double kSoftprobMinHess = 1e-16;         // xgboost's kRtEps floor of the hessian

// xgboost's SoftmaxMultiClassObj for one row: mx = max m_c, e_c = exp(m_c - mx), S = sum e_c
// (ascending), p_c = e_c / S, then g_c = (float)(w (p_c - [c == y])) and
// h_c = (float)fmax(((2 p_c)(1 - p_c)) w, 1e-16). The label is only compared, never an index.
template <int C>
FDX_HD void softprob_row_terms(const double (&m)[C], float y, double w, float (&g)[C], float (&h)[C]) {
  double mx = m[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = m[c] > mx ? m[c] : mx;
  double e[C];
  double S = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = exp(m[c] - mx);
    S += e[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double p = e[c] / S;
    g[c] = (float)(w * (p - ((float)c == y ? 1.0 : 0.0)));
    h[c] = (float)fmax(((2.0 * p) * (1.0 - p)) * w, kSoftprobMinHess);
  }
}

// ---------------------------------------------------------------- descriptors
struct SoftprobGradArgs {
  const double* margin;      // plane c at margin + c * margin_stride, rows [0, N)
  int64_t margin_stride;
  const float* y;            // [N]
  const float* w;            // [N] or nullptr (1.0)
  float* g;                  // plane c at g + c * g_stride: exactly rows [0, N) are written
  int64_t g_stride;
  float* h;
  int64_t h_stride;
  int64_t N;
  int num_classes;           // 2 .. kSoftprobMaxClasses
};

template <class V>
struct ClassTreeArgs {
  const int64_t* indptr;     // [rows + 1]
  const int32_t* idx;        // ascending within a row
  const V* val;
  int64_t rows;
  TreeEnsemble trees;        // K = 1: scalar leaf values; the tree weights are not read
  const int32_t* tree_class; // [num_trees], each 0 .. num_classes - 1
  int num_classes;           // 2 .. kSoftprobMaxClasses
  bool cmp_less;
  double* out;               // [rows, num_classes]
};

void launch_softprob_grad(const SoftprobGradArgs& a, hipStream_t stream);
void softprob_grad_cpu(const SoftprobGradArgs& a, int threads);
template <class V> void launch_score_class_trees(const ClassTreeArgs<V>& a, hipStream_t stream);
template <class V> void score_class_trees_cpu(const ClassTreeArgs<V>& a, int threads);

}  // namespace fdx
