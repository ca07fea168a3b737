// Multinomial logistic regression kernel for gfx950 (contract in mlr.h): one launch is one function
// evaluation on a row shard.
//
// A workgroup of four waves owns a contiguous chunk of rows, a wave one row at a time. The wave
// reads the row's entries lane-strided and coalesced, keeps the C partial margins of a lane in
// registers (C is a template parameter), sums them with the xor butterfly as nb_score does, and
// every lane then holds the row's C margins and computes the row terms (uniform over the wave).
// It walks the same entries again (they are in L1 / L2) and adds the C terms rint(x r_c 2^k) of an
// entry: a feature of the hot set (slot_of[f] < hot_slots) adds into the workgroup's int64 LDS
// table [H][C] with a 64-bit LDS atomic, every other entry goes straight to a global integer
// atomic; zero terms are skipped. The table's non-zero slots are flushed with 64-bit integer global
// atomics when the chunk is done. The intercept sums and the loss are summed per wave in registers,
// then in LDS, and leave the workgroup as C + 1 global atomics. Integer adds commute, so the hot
// set, the chunk size and the grid change the speed only.
#include <stdexcept>

#include "mlr.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ double mlr_wave_sum(double v) {
#pragma unroll
  for (int o = kNbWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kNbWave);
  return v;
}

template <class V, int C>
__global__ __launch_bounds__(kNbBlock) void mlr_eval_kernel(MlrArgs<V> a) {
  extern __shared__ u64 table[];                 // [hot_slots][C]
  __shared__ u64 sums_s[kNbMaxClasses + 1];      // intercept sums, then the loss
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  const int H = a.hot_slots;
  const int slots = C * H;
  for (int i = tid; i < slots; i += kNbBlock) table[i] = 0;
  if (tid <= C) sums_s[tid] = 0;
  __syncthreads();

  const int64_t r0 = (int64_t)blockIdx.x * a.chunk_rows;
  const int64_t r1 = r0 + a.chunk_rows < a.rows ? r0 + a.chunk_rows : a.rows;
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
    for (int c = 0; c < C; ++c) m[c] = mlr_wave_sum(m[c]) + bias[c];
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
      const int slot = H ? (int)a.slot_of[f] : (int)kNbCold;
      u64* const dst = slot < H ? table + slot * C : G + (int64_t)f * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const u64 q = (u64)nb_quant(x * res[c], a.k);
        if (q != 0) atomicAdd(dst + c, q);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (gb[c]) atomicAdd(&sums_s[c], gb[c]);
    if (lossq) atomicAdd(&sums_s[C], lossq);
  }
  // every writer stores the same value into its half of the flag word
  if (clamped_any) reinterpret_cast<int32_t*>(a.flag)[0] = 1;
  if (bad) reinterpret_cast<int32_t*>(a.flag)[1] = 1;
  __syncthreads();
  for (int i = tid; i < slots; i += kNbBlock) {
    const u64 v = table[i];
    if (v == 0) continue;
    const int slot = i / C;
    const int32_t f = a.hot_feat[slot];
    if ((uint32_t)f < (uint32_t)a.F) atomicAdd(G + (int64_t)f * C + (i - slot * C), v);
  }
  if (tid <= C && sums_s[tid]) {
    // gbq [C] and lossq [1] are adjacent in the block only by the caller's choice: address each
    atomicAdd(reinterpret_cast<u64*>(tid < C ? a.gbq + tid : a.lossq), sums_s[tid]);
  }
}

template <class V, int C>
void launch_c(const MlrArgs<V>& a, hipStream_t stream) {
  const size_t lds = (size_t)C * a.hot_slots * sizeof(u64);
  const unsigned grid = (unsigned)nb_chunks(a.rows, a.chunk_rows);
  hipLaunchKernelGGL((mlr_eval_kernel<V, C>), dim3(grid), dim3(kNbBlock), lds, stream, a);
}

}  // namespace

template <class V>
void launch_mlr_eval(const MlrArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  if (a.num_classes < 2 || a.num_classes > kNbMaxClasses || a.chunk_rows < 1 || a.hot_slots < 0 ||
      (int64_t)a.num_classes * a.hot_slots * 8 > kNbMaxTableBytes)
    throw std::runtime_error("fdx mlr_eval: classes, chunk or hot set out of range");
  switch (a.num_classes) {
    case 2: launch_c<V, 2>(a, stream); break;
    case 3: launch_c<V, 3>(a, stream); break;
    case 4: launch_c<V, 4>(a, stream); break;
    case 5: launch_c<V, 5>(a, stream); break;
    case 6: launch_c<V, 6>(a, stream); break;
    case 7: launch_c<V, 7>(a, stream); break;
    default: launch_c<V, 8>(a, stream); break;
  }
}
template void launch_mlr_eval<float>(const MlrArgs<float>&, hipStream_t);
template void launch_mlr_eval<double>(const MlrArgs<double>&, hipStream_t);

}  // namespace fdx
