// Naive Bayes kernels for gfx950 (contracts in nb.h).
//
// nb_sums: the fixed-point row pass of fixedpoint.h with a class-major table [C][H]: a row adds to
// its own class only, one walk over its entries.
//
// nb_score: a wave per row; one gather of W[f][0 .. C) brings every class of an entry, the C
// partials of a lane stay in registers (C is a template parameter).
#include <stdexcept>

#include "nb.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = fx_u64;

template <class V>
__global__ __launch_bounds__(kNbBlock) void nb_sums_kernel(NbSumArgs<V> a) {
  extern __shared__ u64 table[];                 // [num_classes][hot_slots]
  __shared__ u64 wq_s[kNbMaxClasses], cnt_s[kNbMaxClasses];
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  const int C = a.num_classes, H = a.hot_slots;
  fx_table_zero(table, C * H);
  if (tid < kNbMaxClasses) { wq_s[tid] = 0; cnt_s[tid] = 0; }
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  // per-wave sums of the weights and the rows of each class (the class is uniform over a wave)
  u64 wq[kNbMaxClasses], cnt[kNbMaxClasses];
#pragma unroll
  for (int c = 0; c < kNbMaxClasses; ++c) { wq[c] = 0; cnt[c] = 0; }
  bool bad = false;
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const int c = nb_label(a.labels[r], C);
    const double w = a.weights ? a.weights[r] : 1.0;
    if (c < 0 || !nb_weight_ok(w)) { bad = true; continue; }
    const u64 qw = (u64)nb_quant(w, a.kw);
#pragma unroll
    for (int cc = 0; cc < kNbMaxClasses; ++cc) {
      wq[cc] += cc == c ? qw : 0;
      cnt[cc] += cc == c ? 1 : 0;
    }
    u64* const g_row = reinterpret_cast<u64*>(a.S) + (int64_t)c * a.F;
    u64* const t_row = table + c * H;
    const int64_t e = a.indptr[r + 1];
    for (int64_t j = a.indptr[r] + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];
      const double x = (double)a.val[j];
      if ((uint32_t)f >= (uint32_t)a.F || !nb_value_ok(x, a.bernoulli)) { bad = true; continue; }
      const u64 q = (u64)nb_quant(w * x, a.k);
      if (q == 0) continue;
      const int slot = fx_slot(a, f);             // two atomics: a selected pointer would make one flat atomic
      if (slot < H) atomicAdd(&t_row[slot], q);
      else atomicAdd(&g_row[f], q);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kNbMaxClasses; ++c)
      if (cnt[c]) { atomicAdd(&wq_s[c], wq[c]); atomicAdd(&cnt_s[c], cnt[c]); }
  }
  if (bad) *a.flag = 1;                          // every writer stores the same value
  __syncthreads();
  fx_flush_rows(a, table, reinterpret_cast<u64*>(a.S), a.F, C);
  if (tid < C && cnt_s[tid]) {
    atomicAdd(reinterpret_cast<u64*>(a.Wq) + tid, wq_s[tid]);
    atomicAdd(reinterpret_cast<u64*>(a.cnt) + tid, cnt_s[tid]);
  }
}

template <class V, int C>
__global__ __launch_bounds__(kNbBlock) void nb_score_kernel(NbScoreArgs<V> a) {
  const int lane = threadIdx.x & (kNbWave - 1);
  const int64_t r = (int64_t)blockIdx.x * kNbWaves + threadIdx.x / kNbWave;
  if (r >= a.rows) return;
  double part[C];
#pragma unroll
  for (int c = 0; c < C; ++c) part[c] = 0.0;
  const int64_t e = a.indptr[r + 1];
  for (int64_t j = a.indptr[r] + lane; j < e; j += kNbWave) {
    const int32_t f = a.idx[j];
    if ((uint32_t)f >= (uint32_t)a.F) continue;
    const double x = (double)a.val[j];
    const double* w = a.W + (int64_t)f * C;
#pragma unroll
    for (int c = 0; c < C; ++c) part[c] += x * w[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) part[c] = fx_wave_sum(part[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) a.out[r * C + c] = part[c] + a.b[c];
  }
}

template <class V, int C>
void launch_score_c(const NbScoreArgs<V>& a, hipStream_t stream) {
  const unsigned grid = (unsigned)((a.rows + kNbWaves - 1) / kNbWaves);
  hipLaunchKernelGGL((nb_score_kernel<V, C>), dim3(grid), dim3(kNbBlock), 0, stream, a);
}

}  // namespace

template <class V>
void launch_nb_sums(const NbSumArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  const FxLaunch l = fx_launch("nb_sums", a.num_classes, 2, a, a.rows);
  hipLaunchKernelGGL(nb_sums_kernel<V>, dim3(l.grid), dim3(kNbBlock), l.lds, stream, a);
}
template void launch_nb_sums<float>(const NbSumArgs<float>&, hipStream_t);
template void launch_nb_sums<double>(const NbSumArgs<double>&, hipStream_t);

template <class V>
void launch_nb_score(const NbScoreArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  switch (a.num_classes) {
    case 2: launch_score_c<V, 2>(a, stream); break;
    case 3: launch_score_c<V, 3>(a, stream); break;
    case 4: launch_score_c<V, 4>(a, stream); break;
    case 5: launch_score_c<V, 5>(a, stream); break;
    case 6: launch_score_c<V, 6>(a, stream); break;
    case 7: launch_score_c<V, 7>(a, stream); break;
    case 8: launch_score_c<V, 8>(a, stream); break;
    default: throw std::runtime_error("fdx nb_score: classes out of range");
  }
}
template void launch_nb_score<float>(const NbScoreArgs<float>&, hipStream_t);
template void launch_nb_score<double>(const NbScoreArgs<double>&, hipStream_t);

}  // namespace fdx
