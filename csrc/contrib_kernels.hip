// Per-row feature contributions (exact path-dependent TreeSHAP) for gfx950, wave64.
//
// Summation order (the contract; contrib_cpu.cpp follows it operation for operation, so device and
// host agree bitwise, and the result does not depend on grid size, thread count or run):
//   * the order is defined statically on the path table: the elements of a slot (= used feature)
//     are sorted by path;
//   * a slot's elements are cut into blocks of B = kContribBlockElems consecutive elements; a
//     block's terms are added sequentially, in element order, to 0.0;
//   * a slot's block sums are added sequentially in block order, starting from the first block's;
//   * every term is contrib_term (contrib.h), evaluated identically on both sides.
// No atomics anywhere: every output and scratch word has exactly one writer.
//
// One launch handles a tile of <= kContribRowsPerTile rows in four kernels; every lane owns one
// row, so everything read from the path table (~1 MB for 100 trees of depth 6, L2 resident) is
// uniform across a wave and every scratch access is coalesced (scratch is row-minor):
//   gather    wave per row: xs[slot][row] = the row's value of each used feature (else the 0.0
//             the caller wrote), found by binary search of the entry's index in features[]
//   masks     lane per (row, path) in chunks of kContribPathsPerChunk paths: the path's o bits
//   partials  lane per (row, block of B elements): the block sum
//   finish    lane per (row, slot): the slot's block sums in order -> out[row][slot]
#include "contrib.h"
#include "ops.h"
#include "scoring.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {
constexpr int kWave = 64;
constexpr int kBlock = kContribRowsPerGroup;
constexpr int64_t kRT = kContribRowsPerTile;

template <class V>
__global__ __launch_bounds__(kBlock) void contrib_gather_kernel(ContribArgs<V> a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (r >= a.rows) return;
  for (int64_t j = a.indptr[r] + lane; j < a.indptr[r + 1]; j += kWave) {
    const int32_t s = sorted_find(a.p.features, a.p.U, a.idx[j]);
    if (s >= 0) a.xs[(int64_t)s * kRT + r] = (double)a.val[j];
  }
}

template <class V>
__global__ __launch_bounds__(kBlock) void contrib_masks_kernel(ContribArgs<V> a) {
  const int64_t r = (int64_t)blockIdx.y * kBlock + threadIdx.x;
  if (r >= a.rows) return;
  const ContribPaths& t = a.p;
  const int32_t p0 = (int32_t)blockIdx.x * kContribPathsPerChunk;
  const int32_t p1 = p0 + kContribPathsPerChunk < t.P ? p0 + kContribPathsPerChunk : t.P;
  for (int32_t p = p0; p < p1; ++p) {
    uint32_t mask = 0;
    const int32_t e0 = t.path_ptr[p], e1 = t.path_ptr[p + 1];
    for (int32_t e = e0; e < e1; ++e) {
      const double x = a.xs[(int64_t)t.pe_slot[e] * kRT + r];
      if (contrib_test(x, t.pe_lo[e], t.pe_hi[e], t.cmp_less)) mask |= 1u << (e - e0);
    }
    a.masks[(int64_t)p * kRT + r] = mask;
  }
}

template <class V>
__global__ __launch_bounds__(kBlock) void contrib_partials_kernel(ContribArgs<V> a) {
  const int64_t r = (int64_t)blockIdx.y * kBlock + threadIdx.x;
  if (r >= a.rows) return;
  const ContribPaths& t = a.p;
  const int32_t b = (int32_t)blockIdx.x;
  const int32_t s = t.blk_slot[b];
  const int32_t e0 = t.slot_ptr[s] + (b - t.slot_blk[s]) * kContribBlockElems;
  const int32_t e1 = e0 + kContribBlockElems < t.slot_ptr[s + 1] ? e0 + kContribBlockElems : t.slot_ptr[s + 1];
  double acc = 0.0;
  for (int32_t e = e0; e < e1; ++e) {
    const int32_t p = t.el_path[e];
    const int32_t q = t.path_ptr[p];
    acc += contrib_term(t.pe_z + q, t.path_ptr[p + 1] - q, a.masks[(int64_t)p * kRT + r], t.el_pos[e], t.shapley,
                        t.path_v[p]);
  }
  a.partials[(int64_t)b * kRT + r] = acc;
}

template <class V>
__global__ __launch_bounds__(kBlock) void contrib_finish_kernel(ContribArgs<V> a) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.rows * a.p.U) return;
  const int64_t r = i / a.p.U;
  const int32_t s = (int32_t)(i - r * a.p.U);
  const int32_t b0 = a.p.slot_blk[s], b1 = a.p.slot_blk[s + 1];
  double acc = a.partials[(int64_t)b0 * kRT + r];
  for (int32_t b = b0 + 1; b < b1; ++b) acc += a.partials[(int64_t)b * kRT + r];
  a.out[i] = acc;
}
}  // namespace

template <class V>
void launch_tree_contributions(const ContribArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0 || a.p.U <= 0) return;
  FDX_LANES_CHECK(a.rows <= kRT);
  const unsigned groups = (unsigned)((a.rows + kBlock - 1) / kBlock);
  const unsigned waves = (unsigned)((a.rows + (kBlock / kWave) - 1) / (kBlock / kWave));
  hipLaunchKernelGGL(contrib_gather_kernel<V>, dim3(waves), dim3(kBlock), 0, stream, a);
  const unsigned chunks = (unsigned)((a.p.P + kContribPathsPerChunk - 1) / kContribPathsPerChunk);
  hipLaunchKernelGGL(contrib_masks_kernel<V>, dim3(chunks, groups), dim3(kBlock), 0, stream, a);
  hipLaunchKernelGGL(contrib_partials_kernel<V>, dim3((unsigned)a.p.NB, groups), dim3(kBlock), 0, stream, a);
  const int64_t cells = a.rows * a.p.U;
  hipLaunchKernelGGL(contrib_finish_kernel<V>, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     stream, a);
}
template void launch_tree_contributions<float>(const ContribArgs<float>&, hipStream_t);
template void launch_tree_contributions<double>(const ContribArgs<double>&, hipStream_t);

}  // namespace fdx
