// Multi-class gradient boosting kernels for gfx950 (contract in softprob.h).
//
// softprob_grad: one row per lane. Lane i of a workgroup reads row r of each of the C margin planes
// (consecutive lanes read consecutive doubles: every plane access is coalesced), keeps the C margins
// and exponentials in registers (C is a template parameter), and writes row r of the 2 C fp32
// planes. Rows past N are never touched.
//
// score_class_trees: one 64-lane wavefront per row, as score_csr_kernel; the class select is an
// unrolled compare chain over the C register partials, the reduction the xor butterfly.
#include "softprob.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

template <int C>
__global__ __launch_bounds__(kSoftprobBlock) void softprob_grad_kernel(SoftprobGradArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kSoftprobBlock + threadIdx.x;
  if (r >= a.N) return;
  double m[C];
#pragma unroll
  for (int c = 0; c < C; ++c) m[c] = a.margin[(int64_t)c * a.margin_stride + r];
  const float y = a.y[r];
  const double w = a.w ? (double)a.w[r] : 1.0;
  float g[C], h[C];
  softprob_row_terms<C>(m, y, w, g, h);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    a.g[(int64_t)c * a.g_stride + r] = g[c];
    a.h[(int64_t)c * a.h_stride + r] = h[c];
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kSoftprobWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kSoftprobWave);
  return v;
}

// (score_csr_kernel's row binary search)
template <class V>
__device__ __forceinline__ double row_lookup(const int32_t* idx, const V* val, int64_t a, int64_t b, int32_t f) {
  int64_t lo = a, hi = b - 1;
  while (lo <= hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t k = idx[mid];
    if (k == f) return (double)val[mid];
    if (k < f) lo = mid + 1; else hi = mid - 1;
  }
  return 0.0;
}

template <class V, int C>
__global__ __launch_bounds__(kSoftprobBlock) void score_class_trees_kernel(ClassTreeArgs<V> a) {
  const int lane = threadIdx.x & (kSoftprobWave - 1);
  const int64_t r = (int64_t)blockIdx.x * (kSoftprobBlock / kSoftprobWave) + threadIdx.x / kSoftprobWave;
  if (r >= a.rows) return;            // (whole waves leave: the shuffles below see 64 lanes)
  const int64_t s = a.indptr[r], e = a.indptr[r + 1];
  const TreeEnsemble& te = a.trees;
  auto lookup = [&](int32_t f) { return row_lookup(a.idx, a.val, s, e, f); };
  double part[C];
#pragma unroll
  for (int c = 0; c < C; ++c) part[c] = 0.0;
  for (int t = lane; t < te.num_trees; t += kSoftprobWave) {
    const int32_t leaf = tree_find_leaf(te, te.roots[t], a.cmp_less, lookup);
    const double v = te.leaf[leaf];
    const int32_t k = a.tree_class[t];
#pragma unroll
    for (int c = 0; c < C; ++c) part[c] += (k == c) ? v : 0.0;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) part[c] = wave_sum(part[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) a.out[r * C + c] = part[c];
  }
}

template <int C>
void grad_c(const SoftprobGradArgs& a, hipStream_t stream) {
  const unsigned grid = (unsigned)((a.N + kSoftprobBlock - 1) / kSoftprobBlock);
  hipLaunchKernelGGL(softprob_grad_kernel<C>, dim3(grid), dim3(kSoftprobBlock), 0, stream, a);
}

template <class V, int C>
void score_c(const ClassTreeArgs<V>& a, hipStream_t stream) {
  constexpr int kRows = kSoftprobBlock / kSoftprobWave;
  const unsigned grid = (unsigned)((a.rows + kRows - 1) / kRows);
  hipLaunchKernelGGL((score_class_trees_kernel<V, C>), dim3(grid), dim3(kSoftprobBlock), 0, stream, a);
}

}  // namespace

void launch_softprob_grad(const SoftprobGradArgs& a, hipStream_t stream) {
  if (a.N <= 0) return;
  switch (a.num_classes) {
    case 2: grad_c<2>(a, stream); break;
    case 3: grad_c<3>(a, stream); break;
    case 4: grad_c<4>(a, stream); break;
    case 5: grad_c<5>(a, stream); break;
    case 6: grad_c<6>(a, stream); break;
    case 7: grad_c<7>(a, stream); break;
    case 8: grad_c<8>(a, stream); break;
    default: break;          // (the bindings reject every other class count before this)
  }
}

template <class V>
void launch_score_class_trees(const ClassTreeArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  switch (a.num_classes) {
    case 2: score_c<V, 2>(a, stream); break;
    case 3: score_c<V, 3>(a, stream); break;
    case 4: score_c<V, 4>(a, stream); break;
    case 5: score_c<V, 5>(a, stream); break;
    case 6: score_c<V, 6>(a, stream); break;
    case 7: score_c<V, 7>(a, stream); break;
    case 8: score_c<V, 8>(a, stream); break;
    default: break;
  }
}
template void launch_score_class_trees<float>(const ClassTreeArgs<float>&, hipStream_t);
template void launch_score_class_trees<double>(const ClassTreeArgs<double>&, hipStream_t);

}  // namespace fdx
