// Validation monitoring of the GBDT trainer: descriptors and the per-element code shared by
// eval_kernels.hip and eval_cpu.cpp, so both sides execute the same operations (fp contraction is
// off in both). Three ops:
//   tree_eval_update  val_margin[r] += leaf value of the leaf row r of a raw-valued CSR reaches in the
//                     device node table of the tree just grown (tree.h level_plan), split test of
//                     the model scorer: left iff x < threshold (cmp_less)
//   eval_sums         logloss / error / weight sums as exact int64 fixed point
//   eval_auc          exact tie-aware AUC as three integers (U2, P, N)
#pragma once
#include <math.h>

#include "common.h"
#include "tree.h"

namespace fdx {

constexpr int kEvalWave = 64;
constexpr int kEvalRowsPerGroup = 4;      // tree_eval_update: one wave per row, 256 lanes per workgroup
constexpr int kEvalMaxGroups = 2048;      // workgroups of a launch (8 per CU of 256 CUs); waves stride over more rows
constexpr int kEvalMaxNodes = 1024;       // node table entries one workgroup resolves into LDS (32 B each)
constexpr int kEvalWaveLoad = kEvalWave;  // entries of a row one wave holds in registers (one per lane)
constexpr int kEvalAucTile = 256;         // sorted elements per workgroup of the AUC kernels (one per lane)
constexpr int kEvalReduceBlock = 256;     // lanes of a reduction workgroup (eval_sums, AUC tile scans)
constexpr int kEvalMaxWalk = 64;          // bound on a root-to-leaf walk (a malformed table cannot hang a wave)

// The node table of one tree (LevelState arena) plus what maps its (active feature, bin) splits
// back to raw feature values. All arrays live in the caller's memory space.
struct EvalTree {
  const int32_t* feat;        // [max_nodes] active feature of an inner node
  const int32_t* bin;         // [max_nodes]
  const int32_t* left;        // [max_nodes]
  const int32_t* right;       // [max_nodes]
  const uint8_t* leaf;        // [max_nodes]
  const int64_t* stats;       // [max_nodes, 2] quantised (G, H)
  const int32_t* kexp;        // [2]
  const int64_t* fid_orig;    // [Fa] active feature -> original feature id
  const int64_t* boff;        // [Fa + 1] active feature -> first threshold
  const double* thresholds;   // [TB]
  int32_t max_nodes;
  int64_t Fa, TB;             // bounds of the two maps: a table that points outside ends the walk
  double eta, lambda, mds;
};

template <class V>
struct TreeEvalArgs {
  const int64_t* indptr;      // [rows + 1]
  const int32_t* idx;         // sorted per row
  const V* val;
  int64_t rows;
  EvalTree t;
  double* margin;             // [rows]
};

FDX_HD bool eval_is_inner(const EvalTree& t, int32_t n) {
  return !t.leaf[n] && t.left[n] >= 0 && t.feat[n] >= 0 && t.feat[n] < t.Fa;
}

FDX_HD int32_t eval_next(const EvalTree& t, int32_t n, double x) {
  const int64_t j = t.boff[t.feat[n]] + t.bin[n];
  if (j < 0 || j >= t.TB) return -1;
  const int32_t c = x < t.thresholds[j] ? t.left[n] : t.right[n];
  return (c < 0 || c >= t.max_nodes) ? -1 : c;      // (-1: a malformed table ends the walk)
}

FDX_HD double eval_leaf(const EvalTree& t, int32_t n) {
  return leaf_value(t.stats[2 * n], t.stats[2 * n + 1], t.kexp[0], t.kexp[1], t.eta, t.lambda, t.mds);
}

// ---------------------------------------------------------------- logloss / error sums
inline int eval_ceil_log2(double v) {
  int c = 0;
  while (c < 62 && (double)(1ull << c) < v) ++c;
  return c;
}

// Fixed-point exponent of the metric sums: every term w * l is <= w_max * 2^6 (l <= -log(1e-16) < 37),
// so N terms of rint(term * 2^k) stay below 2^62.
inline int eval_sum_kexp(int64_t n_global, double w_max) {
  const int k = 56 - eval_ceil_log2((double)(n_global > 2 ? n_global : 2)) - eval_ceil_log2(w_max > 1.0 ? w_max : 1.0);
  return k < 40 ? k : 40;
}

struct EvalSumArgs {
  const double* margin;
  const float* label;
  const float* weight;   // may be null
  int64_t n;
  double scale;          // 2^k
  int64_t* out;          // [3]: logloss, error, weight sums (added to: zeroed by the caller)
};

struct EvalTerms {
  int64_t l, e, w;
};

FDX_HD EvalTerms eval_terms(double m, float label, double w, double scale) {
  const double y = label > 0.5f ? 1.0 : 0.0;
  const double p = 1.0 / (1.0 + exp(-m));
  const double pl = p > 1e-16 ? p : 1e-16;
  const double ql = (1.0 - p) > 1e-16 ? (1.0 - p) : 1e-16;
  const double l = -y * log(pl) - (1.0 - y) * log(ql);
  const double e = ((p > 0.5) != (y > 0.5)) ? 1.0 : 0.0;
  EvalTerms t;
  t.l = (int64_t)rint((w * l) * scale);
  t.e = (int64_t)rint((w * e) * scale);
  t.w = (int64_t)rint(w * scale);
  return t;
}

// ---------------------------------------------------------------- AUC
// Order-preserving key of an fp64 margin (-0.0 sorts with +0.0).
FDX_HD uint64_t eval_auc_key(double m) {
  union { double d; uint64_t u; } c;
  c.d = m == 0.0 ? 0.0 : m;
  return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}

}  // namespace fdx
