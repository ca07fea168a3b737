// KMeans kernels for gfx950 (contracts in km.h).
//
// km_step: the fixed-point row pass of fixedpoint.h. A workgroup of four waves owns a contiguous
// chunk of rows, a wave one row at a time. The distance walk is mlr_eval's first walk, once per tile
// of kKmTile centers: the wave reads the row's entries lane-strided and coalesced, a lane keeps the
// tile's partial dots in registers, the xor butterfly sums them, and every lane then holds the
// tile's distances and updates the running (least distance, its cluster), uniform over the wave. The
// tile loop runs over the runtime Kp / kKmTile; a row's entries are re-read from L1 / L2 per tile.
// The squared norm of the row comes from the first tile's walk. The accumulate walk is nb_sums':
// one term per entry into the class-major table [K][H] or S, the class being the cluster the row
// was just assigned to. Lane c of a wave keeps the weight sum and the row count of cluster c in
// registers (K <= 64), the cost is uniform over the wave; they go to LDS, then one global atomic each.
//
// km_centers: a workgroup per cluster, lr_reduce's shape: lane t adds features t, t + 256, ...
// ascending, then an LDS tree of fixed shape.
#include <stdexcept>

#include "km.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = fx_u64;

template <class V, int M>
__global__ __launch_bounds__(kNbBlock) void km_step_kernel(KmStepArgs<V> a) {
  extern __shared__ u64 table[];                 // [K][hot_slots], unused without S
  __shared__ u64 wq_s[kKmMaxK], cnt_s[kKmMaxK], cost_s;
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  const int K = a.K, Kp = a.Kp, H = a.hot_slots;
  const bool sums = a.S != nullptr;
  fx_table_zero(table, sums ? K * H : 0);
  if (tid < kKmMaxK) { wq_s[tid] = 0; cnt_s[tid] = 0; }
  if (tid == 0) cost_s = 0;
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  u64 wq = 0, cnt = 0;                           // of cluster `lane`
  u64 costq = 0;                                 // uniform over the wave
  bool bad = false;
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !nb_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double xn = 0.0, nrm = 0.0, best_d = 0.0;
    int best_c = 0;
    for (int t = 0; t < Kp; t += kKmTile) {
      double part[kKmTile];
#pragma unroll
      for (int i = 0; i < kKmTile; ++i) part[i] = 0.0;
      double xp = 0.0;
      for (int64_t j = s + lane; j < e; j += kNbWave) {
        const int32_t f = a.idx[j];
        if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
        const double x = (double)a.val[j];
        const double* ct = a.CT + (int64_t)f * Kp + t;
        if (t == 0) {
          bad_row |= !km_value_ok(x);
          xp += x * x;
        }
#pragma unroll
        for (int i = 0; i < kKmTile; ++i) part[i] += x * ct[i];
      }
      if (t == 0) {                              // the first walk has seen every entry of the row
        xn = fx_wave_sum(xp);
        bad_row = __any(bad_row) || !km_norm_ok(xn, M);
        if (bad_row) break;                      // uniform over the wave
        nrm = sqrt(xn);
      }
#pragma unroll
      for (int i = 0; i < kKmTile; ++i) {
        const double dot = fx_wave_sum(part[i]);
        const int c = t + i;
        if (c < K) {                             // padding columns never compete
          const double d = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c], dot);
          if (c == 0 || d < best_d) { best_d = d; best_c = c; }
        }
      }
    }
    if (bad_row) {
      bad = true;
      if (lane == 0) {
        if (a.assign) a.assign[r] = -1;
        if (a.dist) a.dist[r] = 0.0;
      }
      continue;
    }
    const int c = best_c;                        // in [0, K): c == 0 opens the search, c < K guards every update
    if (lane == c) { wq += (u64)nb_quant(w, a.kw); cnt += 1; }
    costq += (u64)nb_quant(w * best_d, a.kc);
    if (lane == 0) {
      if (a.assign) a.assign[r] = c;
      if (a.dist) a.dist[r] = best_d;
    }
    if (!sums) continue;
    const double sx = km_row_scale(M, w, nrm);
    u64* const g_row = reinterpret_cast<u64*>(a.S) + (int64_t)c * a.F;
    u64* const t_row = table + c * H;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];                // in range: the first walk checked every entry of this row
      const u64 q = (u64)nb_quant(sx * (double)a.val[j], a.k);
      if (q == 0) continue;
      const int slot = fx_slot(a, f);             // two atomics: a selected pointer would make one flat atomic
      if (slot < H) atomicAdd(&t_row[slot], q);
      else atomicAdd(&g_row[f], q);
    }
  }
  if (cnt) { atomicAdd(&wq_s[lane], wq); atomicAdd(&cnt_s[lane], cnt); }   // cnt != 0 only in lanes < K
  if (lane == 0) fx_sum_to_lds(&cost_s, costq);
  if (bad) *a.flag = 1;                          // every writer stores the same value
  __syncthreads();
  if (sums) fx_flush_rows(a, table, reinterpret_cast<u64*>(a.S), a.F, K);
  if (tid < K && cnt_s[tid]) {
    atomicAdd(reinterpret_cast<u64*>(a.Wq) + tid, wq_s[tid]);
    atomicAdd(reinterpret_cast<u64*>(a.cnt) + tid, cnt_s[tid]);
  }
  if (tid == 0) fx_sum_to_global(a.costq, cost_s);
}

// s[0] = sum of the kKmCentersBlock slots, in the order of km_tree_host; every lane calls it
__device__ __forceinline__ double km_tree(double* s, double v) {
  __syncthreads();                               // the previous sum has been read
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kKmCentersBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(kKmCentersBlock) void km_centers_kernel(KmCentersArgs a) {
  __shared__ double s[kKmCentersBlock];
  const int c = blockIdx.x, t = threadIdx.x;      // c < K: the grid is K workgroups
  const int64_t Kp = a.Kp;
  const int64_t wq = a.Wq[c];
  const bool keep = wq == 0;                      // an empty cluster keeps its center
  const double W = ldexp((double)wq, -a.kw);
  const int64_t* S = a.S + (int64_t)c * a.F;
  double inv = 1.0;
  if (!keep && a.measure == kKmCosine) {
    double acc = 0.0;
    for (int32_t f = t; f < a.F; f += kKmCentersBlock) {
      const double m = km_mean(S[f], a.k, W);
      acc += m * m;
    }
    inv = sqrt(km_tree(s, acc));
    if (inv == 0.0) inv = 1.0;                    // a mean of zeros stays
  }
  double nn = 0.0, mv = 0.0;
  for (int32_t f = t; f < a.F; f += kKmCentersBlock) {
    const double old = a.CT_old[f * Kp + c];
    double v = old;
    if (!keep) {
      v = km_mean(S[f], a.k, W);
      if (a.measure == kKmCosine) v = v / inv;
    }
    a.CT_new[f * Kp + c] = v;
    nn += v * v;
    const double d = v - old;
    mv += d * d;
  }
  nn = km_tree(s, nn);
  mv = km_tree(s, mv);
  if (t == 0) {
    a.cn_new[c] = nn;
    a.moved2[c] = mv;
  }
}

template <class V, int M>
void launch_m(const KmStepArgs<V>& a, hipStream_t stream) {
  const FxLaunch l = fx_launch("km_step", a.K, 2, a, a.rows, kKmMaxK, kKmMaxTableBytes);
  hipLaunchKernelGGL((km_step_kernel<V, M>), dim3(l.grid), dim3(kNbBlock), a.S ? l.lds : 0, stream, a);
}

}  // namespace

template <class V>
void launch_km_step(const KmStepArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  if (a.Kp != km_padded(a.K)) throw std::runtime_error("fdx km_step: Kp is K rounded up to the tile");
  switch (a.measure) {
    case kKmEuclidean: launch_m<V, kKmEuclidean>(a, stream); break;
    case kKmCosine: launch_m<V, kKmCosine>(a, stream); break;
    default: throw std::runtime_error("fdx km_step: unknown measure");
  }
}
template void launch_km_step<float>(const KmStepArgs<float>&, hipStream_t);
template void launch_km_step<double>(const KmStepArgs<double>&, hipStream_t);

void launch_km_centers(const KmCentersArgs& a, hipStream_t stream) {
  if (a.K < 2 || a.K > kKmMaxK || a.Kp != km_padded(a.K) || a.F < 1)
    throw std::runtime_error("fdx km_centers: K or F out of range");
  hipLaunchKernelGGL(km_centers_kernel, dim3((unsigned)a.K), dim3(kKmCentersBlock), 0, stream, a);
}

}  // namespace fdx
