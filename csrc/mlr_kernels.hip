// Multinomial logistic regression kernel for gfx950 (contract in mlr.h): one launch is one function
// evaluation on a row shard.
//
// A workgroup of four waves owns a contiguous chunk of rows, a wave one row at a time. The wave
// reads the row's entries lane-strided and coalesced, keeps the C partial margins of a lane in
// registers (C is a template parameter), sums them with the xor butterfly as nb_score does, and
// every lane then holds the row's C margins and computes the row terms (uniform over the wave).
// It walks the same entries again (they are in L1 / L2) and adds the C terms rint(x r_c 2^k) of an
// entry into the feature-major table [H][C] or Gq (the fixed-point row pass of fixedpoint.h); zero
// terms are skipped. The intercept sums and the loss are the scalar sums: C + 1 global atomics.
#include <stdexcept>

#include "mlr.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = fx_u64;

template <class V, int C>
__global__ __launch_bounds__(kNbBlock) void mlr_eval_kernel(MlrArgs<V> a) {
  extern __shared__ u64 table[];                 // [hot_slots][C]
  __shared__ u64 sums_s[kNbMaxClasses + 1];      // intercept sums, then the loss
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  fx_table_zero(table, C * a.hot_slots);
  if (tid <= C) sums_s[tid] = 0;
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  double bias[C];
#pragma unroll
  for (int c = 0; c < C; ++c) bias[c] = a.b[c];
  u64 gb[C], lossq = 0;                          // uniform over the wave
#pragma unroll
  for (int c = 0; c < C; ++c) gb[c] = 0;
  bool bad = false, clamped_any = false;
  u64* const G = reinterpret_cast<u64*>(a.Gq);
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const int y = nb_label(a.labels[r], C);
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = y < 0 || !mlr_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double m[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = 0.0;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      bad_row |= !mlr_value_ok(x);
      const double* xs = a.XS + (int64_t)f * C;
#pragma unroll
      for (int c = 0; c < C; ++c) m[c] += x * xs[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = fx_wave_sum(m[c]) + bias[c];
    bad_row = __any(bad_row);
    double res[C];
    double loss = 0.0;
    if (bad_row) {
      bad = true;
#pragma unroll
      for (int c = 0; c < C; ++c) res[c] = 0.0;
    } else {
      bool clamped;
      loss = mlr_row_terms<C>(m, y, w, res, clamped);
      clamped_any |= clamped;
      lossq += (u64)nb_quant(w * loss, a.kl);
#pragma unroll
      for (int c = 0; c < C; ++c) gb[c] += (u64)nb_quant(res[c], a.k);
    }
    if (lane == 0) {
      if (a.margin) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.margin[r * C + c] = m[c];
      }
      if (a.R) {
#pragma unroll
        for (int c = 0; c < C; ++c) a.R[r * C + c] = res[c];
      }
      if (a.loss_row) a.loss_row[r] = loss;
    }
    if (bad_row) continue;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];
      const double x = (double)a.val[j];
      u64* const dst = fx_dst<C>(a, table, G, f);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const u64 q = (u64)nb_quant(x * res[c], a.k);
        if (q != 0) atomicAdd(dst + c, q);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) fx_sum_to_lds(&sums_s[c], gb[c]);
    fx_sum_to_lds(&sums_s[C], lossq);
  }
  fx_flag(a.flag, clamped_any, bad);
  __syncthreads();
  fx_flush<C>(a, table, G, a.F);
  // gbq [C] and lossq [1] are adjacent in the block only by the caller's choice: address each
  if (tid <= C) fx_sum_to_global(tid < C ? a.gbq + tid : a.lossq, sums_s[tid]);
}

template <class V, int C>
void launch_c(const MlrArgs<V>& a, hipStream_t stream) {
  const FxLaunch l = fx_launch("mlr_eval", C, 2, a, a.rows);
  hipLaunchKernelGGL((mlr_eval_kernel<V, C>), dim3(l.grid), dim3(kNbBlock), l.lds, stream, a);
}

}  // namespace

template <class V>
void launch_mlr_eval(const MlrArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  switch (a.num_classes) {
    case 2: launch_c<V, 2>(a, stream); break;
    case 3: launch_c<V, 3>(a, stream); break;
    case 4: launch_c<V, 4>(a, stream); break;
    case 5: launch_c<V, 5>(a, stream); break;
    case 6: launch_c<V, 6>(a, stream); break;
    case 7: launch_c<V, 7>(a, stream); break;
    case 8: launch_c<V, 8>(a, stream); break;
    default: throw std::runtime_error("fdx mlr_eval: classes out of range");
  }
}
template void launch_mlr_eval<float>(const MlrArgs<float>&, hipStream_t);
template void launch_mlr_eval<double>(const MlrArgs<double>&, hipStream_t);

}  // namespace fdx
