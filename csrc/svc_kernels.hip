// Linear SVC (hinge loss) kernel for gfx950 (contract in svc.h): one launch is one function
// evaluation on a row shard.
//
// A workgroup of four waves owns a contiguous chunk of rows, a wave one row at a time. The wave
// reads the row's entries lane-strided and coalesced, sums the lanes' partial margins with the xor
// butterfly as spmv does, and every lane then holds the margin and computes the row terms (uniform
// over the wave). A row inside the margin (residual exactly 0) or with bad input ends there, a
// wave-uniform branch: near the optimum most rows do. Only an active row walks its entries again
// (they are in L1 / L2) and adds rint(x r 2^k) per entry into the table [H] or Gq (the fixed-point
// row pass of fixedpoint.h with C = 1); zero terms are skipped. The intercept sum, the loss and the
// active-row count are the scalar sums: at most three global atomics.
#include <stdexcept>

#include "svc.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = fx_u64;

template <class V>
__global__ __launch_bounds__(kNbBlock) void svc_eval_kernel(SvcArgs<V> a) {
  extern __shared__ u64 table[];                 // [hot_slots]
  __shared__ u64 sums_s[3];                      // gbq, lossq, nact
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  fx_table_zero(table, a.hot_slots);
  if (tid < 3) sums_s[tid] = 0;
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  const double bias = a.b;
  u64 gb = 0, lossq = 0, nact = 0;               // uniform over the wave
  bool bad = false, clamped_any = false;
  u64* const G = reinterpret_cast<u64*>(a.Gq);
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const double y = a.labels[r];
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !svc_label_ok(y) || !mlr_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double m = 0.0;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      bad_row |= !mlr_value_ok(x);
      m += x * a.xs[f];
    }
    m = fx_wave_sum(m) + bias;
    bad_row = __any(bad_row);
    double res = 0.0, loss = 0.0;
    if (bad_row) {
      bad = true;
    } else {
      bool clamped;
      loss = svc_row_terms(m, y, w, res, clamped);
      clamped_any |= clamped;
      lossq += (u64)nb_quant(w * loss, a.kl);
    }
    if (lane == 0) {
      if (a.margin) a.margin[r] = m;
      if (a.r) a.r[r] = res;
      if (a.loss_row) a.loss_row[r] = loss;
    }
    if (res == 0.0) continue;                    // inside the margin, weight 0 or bad input
    gb += (u64)nb_quant(res, a.k);
    nact += 1;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];                // in range: the row is not bad
      const u64 q = (u64)nb_quant((double)a.val[j] * res, a.k);
      if (q == 0) continue;
      atomicAdd(fx_dst<1>(a, table, G, f), q);
    }
  }
  if (lane == 0) {
    fx_sum_to_lds(&sums_s[0], gb);
    fx_sum_to_lds(&sums_s[1], lossq);
    fx_sum_to_lds(&sums_s[2], nact);
  }
  fx_flag(a.flag, clamped_any, bad);
  __syncthreads();
  fx_flush<1>(a, table, G, a.F);
  // the three sums are adjacent in the block only by the caller's choice: address each
  if (tid < 3) fx_sum_to_global(tid == 0 ? a.gbq : tid == 1 ? a.lossq : a.nact, sums_s[tid]);
}

}  // namespace

template <class V>
void launch_svc_eval(const SvcArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  const FxLaunch l = fx_launch("svc_eval", 1, 1, a, a.rows);
  hipLaunchKernelGGL(svc_eval_kernel<V>, dim3(l.grid), dim3(kNbBlock), l.lds, stream, a);
}
template void launch_svc_eval<float>(const SvcArgs<float>&, hipStream_t);
template void launch_svc_eval<double>(const SvcArgs<double>&, hipStream_t);

}  // namespace fdx
