// Bisecting KMeans and silhouette kernels for gfx950 (contracts in clu.h).
//
// Both are km_step's frame (km_kernels.hip): a workgroup of four waves owns a contiguous chunk of
// rows, a wave one row at a time; the row's entries are read lane-strided and coalesced and summed
// with the xor butterfly.
//
// km_group_step: the wave reads group[r] first; a skipped row costs that one read. There is no tile
// loop: one walk gives the squared norm and the W dots against the adjacent columns W g .. (W = 2:
// one 16-byte read per entry), a second walk only with S, into the class-major table [K][H] or S.
// Lane c of a wave keeps Wq, cnt and costq of cluster c in registers (K <= 64); they go to LDS, then
// one global atomic each.
//
// sil_score: km_step's tile loop over the cluster means, the running own and neighbour distances
// uniform over the wave, one coefficient per row; the two sums stay in registers per wave, then LDS,
// then one global atomic each. No table.
#include <stdexcept>

#include "clu.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

using u64 = fx_u64;

template <class V, int M, int W>
__global__ __launch_bounds__(kNbBlock) void km_group_kernel(KmGroupArgs<V> a) {
  extern __shared__ u64 table[];                 // [K][hot_slots], unused without S
  __shared__ u64 wq_s[kKmMaxK], cnt_s[kKmMaxK], cost_s[kKmMaxK];
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  const int K = a.K, Kp = a.Kp, H = a.hot_slots;
  const bool sums = a.S != nullptr;
  fx_table_zero(table, sums ? K * H : 0);
  if (tid < kKmMaxK) { wq_s[tid] = 0; cnt_s[tid] = 0; cost_s[tid] = 0; }
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  u64 wq = 0, cnt = 0, costq = 0;                // of cluster `lane`
  bool bad = false;
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const int g = a.group[r];                    // uniform over the wave
    if (g < 0 || g >= a.G) {                     // skipped, or bad input: nothing else of the row is read
      bad |= g >= 0;
      if (lane == 0) {
        if (a.assign) a.assign[r] = -1;
        if (a.dist) a.dist[r] = 0.0;
      }
      continue;
    }
    const double w = a.weights ? a.weights[r] : 1.0;
    bool bad_row = !nb_weight_ok(w);
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    const int c0 = W * g;                        // c0 + W <= W G <= K
    double xp = 0.0, p0 = 0.0, p1 = 0.0;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];
      if ((uint32_t)f >= (uint32_t)a.F) { bad_row = true; continue; }
      const double x = (double)a.val[j];
      bad_row |= !km_value_ok(x);
      xp += x * x;
      const double* ct = a.CT + (int64_t)f * Kp + c0;
      if (W == 2) {
        const double2 cc = *reinterpret_cast<const double2*>(ct);   // c0 is even, a row of CT a multiple of 64 bytes
        p0 += x * cc.x;
        p1 += x * cc.y;
      } else {
        p0 += x * ct[0];
      }
    }
    const double xn = fx_wave_sum(xp);
    bad_row = __any(bad_row) || !km_norm_ok(xn, M);
    if (bad_row) {                               // uniform over the wave
      bad = true;
      if (lane == 0) {
        if (a.assign) a.assign[r] = -1;
        if (a.dist) a.dist[r] = 0.0;
      }
      continue;
    }
    const double nrm = sqrt(xn);
    double d = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c0], fx_wave_sum(p0));
    int c = c0;
    if (W == 2) {
      const double d1 = km_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.cn[c0 + 1], fx_wave_sum(p1));
      if (d1 < d) { d = d1; c = c0 + 1; }        // the left child wins ties
    }
    if (lane == c) {
      wq += (u64)nb_quant(w, a.kw);
      cnt += 1;
      costq += (u64)nb_quant(w * d, a.kc);
    }
    if (lane == 0) {
      if (a.assign) a.assign[r] = c;
      if (a.dist) a.dist[r] = d;
    }
    if (!sums) continue;
    const double sx = km_row_scale(M, w, nrm);
    u64* const g_row = reinterpret_cast<u64*>(a.S) + (int64_t)c * a.F;
    u64* const t_row = table + c * H;
    for (int64_t j = s + lane; j < e; j += kNbWave) {
      const int32_t f = a.idx[j];                // in range: the first walk checked every entry of this row
      const u64 q = (u64)nb_quant(sx * (double)a.val[j], a.k);
      if (q == 0) continue;
      const int slot = fx_slot(a, f);
      if (slot < H) atomicAdd(&t_row[slot], q);
      else atomicAdd(&g_row[f], q);
    }
  }
  if (cnt) {                                     // cnt != 0 only in lanes < K
    atomicAdd(&wq_s[lane], wq);
    atomicAdd(&cnt_s[lane], cnt);
    if (costq) atomicAdd(&cost_s[lane], costq);
  }
  if (bad) *a.flag = 1;                          // every writer stores the same value
  __syncthreads();
  if (sums) fx_flush_rows(a, table, reinterpret_cast<u64*>(a.S), a.F, K);
  if (tid < K && cnt_s[tid]) {
    atomicAdd(reinterpret_cast<u64*>(a.Wq) + tid, wq_s[tid]);
    atomicAdd(reinterpret_cast<u64*>(a.cnt) + tid, cnt_s[tid]);
    fx_sum_to_global(a.costq + tid, cost_s[tid]);
  }
}

template <class V, int M>
__global__ __launch_bounds__(kNbBlock) void sil_score_kernel(SilArgs<V> a) {
  __shared__ u64 sil_s, wq_s;
  const int tid = threadIdx.x, lane = tid & (kNbWave - 1), wave = tid / kNbWave;
  const int K = a.K, Kp = a.Kp;
  if (tid == 0) { sil_s = 0; wq_s = 0; }
  __syncthreads();

  int64_t r0, r1;
  fx_chunk(a, a.rows, r0, r1);
  u64 silq = 0, wq = 0;                          // uniform over the wave
  bool bad = false;
  for (int64_t r = r0 + wave; r < r1; r += kNbWaves) {
    const double w = a.weights ? a.weights[r] : 1.0;
    const int own_c = a.label[r];                // uniform over the wave
    bool bad_row = !nb_weight_ok(w) || (uint32_t)own_c >= (uint32_t)K;
    if (!bad_row) bad_row = !(a.nw[own_c] > 0.0);                  // a label of an absent cluster
    const int64_t s = a.indptr[r], e = a.indptr[r + 1];
    double xn = 0.0, nrm = 0.0, own = 0.0, nb = 0.0;
    bool have_nb = false;
    for (int t = 0; t < Kp && !bad_row; t += kKmTile) {
      double part[kKmTile];
#pragma unroll
      for (int i = 0; i < kKmTile; ++i) part[i] = 0.0;
      double xp = 0.0;
      bool bad_entry = false;
      for (int64_t j = s + lane; j < e; j += kNbWave) {
        const int32_t f = a.idx[j];
        if ((uint32_t)f >= (uint32_t)a.F) { bad_entry = true; continue; }
        const double x = (double)a.val[j];
        const double* mt = a.MT + (int64_t)f * Kp + t;
        if (t == 0) {
          bad_entry |= !km_value_ok(x);
          xp += x * x;
        }
#pragma unroll
        for (int i = 0; i < kKmTile; ++i) part[i] += x * mt[i];
      }
      if (t == 0) {                              // the first walk has seen every entry of the row
        xn = fx_wave_sum(xp);
        bad_row = __any(bad_entry) || !km_norm_ok(xn, M);
        if (bad_row) break;                      // uniform over the wave
        nrm = sqrt(xn);
      }
#pragma unroll
      for (int i = 0; i < kKmTile; ++i) {
        const double dot = fx_wave_sum(part[i]);
        const int c = t + i;
        if (c < K) {                             // padding columns never compete
          const double d = clu_sil_distance(M, xn, nrm, M == kKmCosine ? 0.0 : a.psi[c], dot);
          if (c == own_c) own = d;
          else if (a.nw[c] > 0.0 && (!have_nb || d < nb)) { nb = d; have_nb = true; }
        }
      }
    }
    double sc = 0.0;
    if (!bad_row) {
      bool ok;
      sc = clu_silhouette(a.cnt[own_c], own, nb, a.nw[own_c], w, &ok);
      bad_row = !have_nb || !ok;
    }
    if (bad_row) {
      bad = true;
      if (lane == 0 && a.s) a.s[r] = 0.0;
      continue;
    }
    silq += (u64)nb_quant(w * sc, a.ks);
    wq += (u64)nb_quant(w, a.kw);
    if (lane == 0 && a.s) a.s[r] = sc;
  }
  if (lane == 0) {
    fx_sum_to_lds(&sil_s, silq);
    fx_sum_to_lds(&wq_s, wq);
  }
  if (bad) *a.flag = 1;                          // every writer stores the same value
  __syncthreads();
  if (tid == 0) {
    fx_sum_to_global(a.silq, sil_s);
    fx_sum_to_global(a.wq, wq_s);
  }
}

template <class V, int M, int W>
void launch_group(const KmGroupArgs<V>& a, hipStream_t stream) {
  const FxLaunch l = fx_launch("km_group_step", a.K, 2, a, a.rows, kKmMaxK, kKmMaxTableBytes);
  hipLaunchKernelGGL((km_group_kernel<V, M, W>), dim3(l.grid), dim3(kNbBlock), a.S ? l.lds : 0, stream, a);
}

template <class V, int M>
void launch_group_w(const KmGroupArgs<V>& a, hipStream_t stream) {
  if (a.W == 2) launch_group<V, M, 2>(a, stream);
  else launch_group<V, M, 1>(a, stream);
}

}  // namespace

template <class V>
void launch_km_group_step(const KmGroupArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  if ((a.W != 1 && a.W != 2) || a.G < 1 || a.W * a.G > kKmMaxK || a.K != clu_centers(a.W, a.G) ||
      a.Kp != km_padded(a.K))
    throw std::runtime_error("fdx km_group_step: W, G, K or Kp out of range");
  if (reinterpret_cast<uintptr_t>(a.CT) % 16 != 0) throw std::runtime_error("fdx km_group_step: CT is 16-byte aligned");
  switch (a.measure) {
    case kKmEuclidean: launch_group_w<V, kKmEuclidean>(a, stream); break;
    case kKmCosine: launch_group_w<V, kKmCosine>(a, stream); break;
    default: throw std::runtime_error("fdx km_group_step: unknown measure");
  }
}
template void launch_km_group_step<float>(const KmGroupArgs<float>&, hipStream_t);
template void launch_km_group_step<double>(const KmGroupArgs<double>&, hipStream_t);

template <class V>
void launch_sil_score(const SilArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  if (a.K < 2 || a.K > kKmMaxK || a.Kp != km_padded(a.K) || a.chunk_rows < 1)
    throw std::runtime_error("fdx sil_score: K, Kp or chunk out of range");
  const dim3 grid((unsigned)nb_chunks(a.rows, a.chunk_rows));
  switch (a.measure) {
    case kKmEuclidean: hipLaunchKernelGGL((sil_score_kernel<V, kKmEuclidean>), grid, dim3(kNbBlock), 0, stream, a); break;
    case kKmCosine: hipLaunchKernelGGL((sil_score_kernel<V, kKmCosine>), grid, dim3(kNbBlock), 0, stream, a); break;
    default: throw std::runtime_error("fdx sil_score: unknown measure");
  }
}
template void launch_sil_score<float>(const SilArgs<float>&, hipStream_t);
template void launch_sil_score<double>(const SilArgs<double>&, hipStream_t);

}  // namespace fdx
