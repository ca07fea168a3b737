// Path-dependent TreeSHAP over the path table of an ensemble (ml/tree_model.py ensemble_paths):
// descriptors and the per-element term, shared by contrib_kernels.hip and contrib_cpu.cpp so both
// execute the same sequence of fp64 operations (bitwise agreement; fp contraction is off in both).
#pragma once
#include "common.h"

namespace fdx {

constexpr int kContribMaxDepth = 32;     // distinct features on one path (the o bits fit one uint32)
constexpr int kContribBlockElems = 16;   // B: consecutive elements of one slot summed by one lane
constexpr int kContribPathsPerChunk = 16;   // paths whose masks one workgroup computes for its rows
constexpr int kContribRowsPerGroup = 256;   // rows of one workgroup (one lane per row)
constexpr int kContribRowsPerTile = 1024;   // rows of one launch (bounds the device scratch)

// All arrays live in the caller's memory space. "Element" = one distinct feature on one
// root-to-leaf path; the elements exist twice: path-major (pe_*, for the masks and the term) and
// sorted by (slot, path) (el_*, the summation order).
struct ContribPaths {
  const int32_t* features;   // [U] sorted distinct features of the ensemble (slot -> feature)
  const int32_t* path_ptr;   // [P + 1] path -> its elements in pe_*
  const double* path_v;      // [P] leaf value x tree weight
  const int32_t* pe_slot;    // [E]
  const double* pe_z;        // [E] fraction of the cover that follows the path at this element
  const double* pe_lo;       // [E] merged tests: cmp_less ? lo <= x < hi : lo < x <= hi
  const double* pe_hi;       // [E]
  const int32_t* el_path;    // [E] sorted by (slot, path)
  const int32_t* el_pos;     // [E] position of the element within its path
  const int32_t* slot_ptr;   // [U + 1] slot -> its elements in el_*
  const int32_t* slot_blk;   // [U + 1] slot -> its blocks (ceil(len / B) each)
  const int32_t* blk_slot;   // [NB]
  const double* shapley;     // [33 * 32] shapley[d * 32 + k] = k! (d - k - 1)! / d!
  int32_t U, P, E, NB;
  bool cmp_less;
};

template <class V>
struct ContribArgs {
  const int64_t* indptr;     // [rows + 1] (absolute offsets into idx / val)
  const int32_t* idx;
  const V* val;
  int64_t rows;              // device: <= kContribRowsPerTile
  ContribPaths p;
  double* out;               // [rows * U]
  // device scratch of one row tile (nullptr on the host): row-minor, stride kContribRowsPerTile
  double* xs;                // [U] values of the used features (0.0 where the row has no entry; zeroed by the caller)
  uint32_t* masks;           // [P]
  double* partials;          // [NB]
};

FDX_HD bool contrib_test(double x, double lo, double hi, bool cmp_less) {
  // the conjunction of tree_find_leaf's tests: right-going nodes give lo, left-going nodes hi
  return cmp_less ? (!(x < lo) && (x < hi)) : (!(x <= lo) && (x <= hi));
}

// v * (o_i - z_i) * sum_k shapley[d][k] * c_k, where c_k is the coefficient of y^k in
// prod_{j != i} (z_j + o_j y) (= sum over subsets S of size k of prod_{j in S} o_j prod_{j not in S} z_j).
// The product is expanded element by element in path order, coefficients from high to low.
template <int D>
FDX_HD double contrib_term_n(const double* z, int d, uint32_t mask, int i, const double* w, double v) {
  double c[D];
  c[0] = 1.0;
#pragma unroll
  for (int k = 1; k < D; ++k) c[k] = 0.0;
  int n = 0;   // factors multiplied in so far
#pragma unroll
  for (int j = 0; j < D; ++j) {
    if (j < d && j != i) {
      const double zj = z[j];
      const bool on = (mask >> j) & 1u;
#pragma unroll
      for (int k = D - 1; k >= 1; --k)
        if (D <= 8 || k <= n + 1) c[k] = c[k] * zj + (on ? c[k - 1] : 0.0);   // c[k] == 0 above n + 1
      c[0] = c[0] * zj;
      ++n;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k)
    if (k < d) s += w[k] * c[k];
  const double oi = ((mask >> i) & 1u) ? 1.0 : 0.0;
  return ((oi - z[i]) * s) * v;
}

FDX_HD double contrib_term(const double* z, int d, uint32_t mask, int i, const double* shapley, double v) {
  const double* w = shapley + d * kContribMaxDepth;
  return d <= 8 ? contrib_term_n<8>(z, d, mask, i, w, v) : contrib_term_n<kContribMaxDepth>(z, d, mask, i, w, v);
}

}  // namespace fdx
