// Elastic-net logistic regression kernels for gfx950 (contracts in lr.h, host twins in lr_cpu.cpp).
//
// lr_forward fuses the margin SpMV (one 64-lane wave per row, the lane-strided partial and xor
// butterfly of sparse_kernels.hip::spmv_kernel, so margins are bitwise spmv + b) with the per-row
// log-loss and residual (four lanes of the first wave, one per row), and leaves one partial per
// workgroup. The parameter passes (lr_owlqn_step, lr_pseudo_grad) are grid-stride over pairs of
// fp64 parameters with 16-byte loads and stores. Sums
// never use atomics: per-lane strided sums in ascending order, an LDS tree of fixed shape, one
// partial per workgroup, and lr_reduce (one workgroup) over the partials.
#include "lr.h"
#include "ops.h"

#pragma clang fp contract(off)

namespace fdx {

namespace {

__device__ __forceinline__ double lr_wave_sum(double v) {
#pragma unroll
  for (int o = kLrWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kLrWave);
  return v;
}

// s[0] = sum of the kLrBlock slots, in the order of lr_tree_host; every lane of the workgroup calls it
__device__ __forceinline__ void lr_tree(double* s) {
  __syncthreads();
#pragma unroll
  for (int o = kLrBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
}

template <class V>
__global__ __launch_bounds__(kLrBlock) void lr_forward_kernel(LrForwardArgs<V> a, int64_t P) {
  __shared__ double sm[kLrRowsPerPartial];
  const int lane = threadIdx.x & (kLrWave - 1);
  const int wv = threadIdx.x / kLrWave;
  const int64_t r0 = (int64_t)blockIdx.x * kLrRowsPerPartial;
  const int64_t r = r0 + wv;
  if (r < a.rows) {      // wave-uniform
    double part = 0.0;
    for (int64_t j = a.indptr[r] + lane; j < a.indptr[r + 1]; j += kLrWave) part += (double)a.val[j] * a.xs[a.idx[j]];
    part = lr_wave_sum(part);
    if (lane == 0) sm[wv] = part + a.b[0];
  }
  __syncthreads();
  if (wv != 0) return;
  // the exp / log1p tail of the workgroup's rows runs once, in lanes 0..3 of the first wave, instead
  // of in one lane of each of four waves
  const int64_t row = r0 + lane;
  double wl = 0.0, rr = 0.0;
  if (lane < kLrRowsPerPartial && row < a.rows) {
    const double m = sm[lane];
    const double w = a.w[row];
    const LrRowTerms t = lr_row_terms(m, a.y[row], w);
    a.r[row] = t.r;
    if (a.loss_row) a.loss_row[row] = t.loss;
    if (a.margin) a.margin[row] = m;
    wl = w * t.loss;
    rr = t.r;
  }
  double s0 = 0.0, s1 = 0.0;      // rows added in order, as the host twin does
#pragma unroll
  for (int k = 0; k < kLrRowsPerPartial; ++k) {
    const double u = __shfl(wl, k, kLrWave), v = __shfl(rr, k, kLrWave);
    if (r0 + k < a.rows) { s0 += u; s1 += v; }
  }
  if (lane == 0) {
    a.partials[blockIdx.x] = s0;
    a.partials[P + blockIdx.x] = s1;
  }
}

__global__ __launch_bounds__(kLrReduceBlock) void lr_reduce_kernel(LrReduceArgs a) {
  __shared__ double s[kLrReduceBlock];
  const int t = threadIdx.x;
  for (int64_t k = 0; k < a.K; ++k) {
    const double* p = a.partials + k * a.P;
    double acc = 0.0;
    int64_t i = t;
    // four loads in flight, added in ascending order
    for (; i + 3 * kLrReduceBlock < a.P; i += 4 * kLrReduceBlock) {
      const double v0 = p[i], v1 = p[i + kLrReduceBlock], v2 = p[i + 2 * kLrReduceBlock], v3 = p[i + 3 * kLrReduceBlock];
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; i < a.P; i += kLrReduceBlock) acc += p[i];
    s[t] = acc;
    lr_tree(s);
    if (t == 0) a.out[k] = s[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLrBlock) void lr_owlqn_step_kernel(LrStepArgs a, int64_t G) {
  __shared__ double s[3][kLrBlock];
  const int64_t n = a.F + 1, pairs = (n + 1) / 2, full = a.F / 2;   // pairs below `full` hold coefficients only
  double l1 = 0.0, sq = 0.0, dec = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * kLrBlock + threadIdx.x; p < pairs; p += G * kLrBlock) {
    const int64_t j = 2 * p;
    if (p < full) {
      const double2 x = *reinterpret_cast<const double2*>(a.x + j);
      const double2 d = *reinterpret_cast<const double2*>(a.d + j);
      const double2 xi = *reinterpret_cast<const double2*>(a.xi + j);
      const double2 pg = *reinterpret_cast<const double2*>(a.pg + j);
      const double2 sc = *reinterpret_cast<const double2*>(a.scale + j);
      const LrStepTerms u = lr_step_terms(x.x, d.x, xi.x, pg.x, sc.x, a.t, true);
      const LrStepTerms v = lr_step_terms(x.y, d.y, xi.y, pg.y, sc.y, a.t, true);
      *reinterpret_cast<double2*>(a.x_new + j) = make_double2(u.x_new, v.x_new);
      *reinterpret_cast<double2*>(a.xs_new + j) = make_double2(u.xs_new, v.xs_new);
      l1 += u.l1; sq += u.sq; dec += u.dec;
      l1 += v.l1; sq += v.sq; dec += v.dec;
    } else {
      for (int64_t jj = j; jj < j + 2 && jj < n; ++jj) {
        const bool coef = jj < a.F;
        const LrStepTerms u = lr_step_terms(a.x[jj], a.d[jj], a.xi[jj], a.pg[jj], coef ? a.scale[jj] : 0.0, a.t, coef);
        a.x_new[jj] = u.x_new;
        if (coef) a.xs_new[jj] = u.xs_new;
        l1 += u.l1; sq += u.sq; dec += u.dec;
      }
    }
  }
  s[0][threadIdx.x] = l1;
  s[1][threadIdx.x] = sq;
  s[2][threadIdx.x] = dec;
  __syncthreads();
#pragma unroll
  for (int o = kLrBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s[0][threadIdx.x] += s[0][threadIdx.x + o];
      s[1][threadIdx.x] += s[1][threadIdx.x + o];
      s[2][threadIdx.x] += s[2][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.partials[blockIdx.x] = s[0][0];
    a.partials[G + blockIdx.x] = s[1][0];
    a.partials[2 * G + blockIdx.x] = s[2][0];
  }
}

__global__ __launch_bounds__(kLrBlock) void lr_pseudo_grad_kernel(LrGradArgs a, int64_t G) {
  __shared__ double s[kLrBlock];
  const int64_t n = a.F + 1, pairs = (n + 1) / 2, full = a.F / 2;
  const double* xtr = a.parts + 2;      // 16-byte aligned with parts
  double nn = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * kLrBlock + threadIdx.x; p < pairs; p += G * kLrBlock) {
    const int64_t j = 2 * p;
    if (p < full) {
      const double2 q = *reinterpret_cast<const double2*>(xtr + j);
      const double2 sc = *reinterpret_cast<const double2*>(a.scale + j);
      const double2 x = *reinterpret_cast<const double2*>(a.x + j);
      const LrGradTerms u = lr_grad_terms(q.x, sc.x, a.W, x.x, a.l1, a.l2);
      const LrGradTerms v = lr_grad_terms(q.y, sc.y, a.W, x.y, a.l1, a.l2);
      *reinterpret_cast<double2*>(a.g + j) = make_double2(u.g, v.g);
      *reinterpret_cast<double2*>(a.pg + j) = make_double2(u.pg, v.pg);
      *reinterpret_cast<double2*>(a.xi + j) = make_double2(u.xi, v.xi);
      nn += u.pg * u.pg;
      nn += v.pg * v.pg;
    } else {
      for (int64_t jj = j; jj < j + 2 && jj < n; ++jj) {
        LrGradTerms u;
        if (jj < a.F) {
          u = lr_grad_terms(xtr[jj], a.scale[jj], a.W, a.x[jj], a.l1, a.l2);
        } else {      // intercept: unpenalised, no orthant
          u.g = a.fit_intercept ? a.parts[1] / a.W : 0.0;
          u.pg = u.g;
          u.xi = 0.0;
        }
        a.g[jj] = u.g;
        a.pg[jj] = u.pg;
        a.xi[jj] = u.xi;
        nn += u.pg * u.pg;
      }
    }
  }
  s[threadIdx.x] = nn;
  lr_tree(s);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s[0];
}

}  // namespace

template <class V>
void launch_lr_forward(const LrForwardArgs<V>& a, hipStream_t stream) {
  if (a.rows <= 0) return;
  const int64_t P = lr_forward_partials(a.rows);
  hipLaunchKernelGGL(lr_forward_kernel<V>, dim3((unsigned)P), dim3(kLrBlock), 0, stream, a, P);
}
template void launch_lr_forward<float>(const LrForwardArgs<float>&, hipStream_t);
template void launch_lr_forward<double>(const LrForwardArgs<double>&, hipStream_t);

void launch_lr_reduce(const LrReduceArgs& a, hipStream_t stream) {
  if (a.K <= 0) return;
  hipLaunchKernelGGL(lr_reduce_kernel, dim3(1), dim3(kLrReduceBlock), 0, stream, a);
}

void launch_lr_owlqn_step(const LrStepArgs& a, hipStream_t stream) {
  const int64_t G = lr_param_groups(a.F + 1);
  hipLaunchKernelGGL(lr_owlqn_step_kernel, dim3((unsigned)G), dim3(kLrBlock), 0, stream, a, G);
}

void launch_lr_pseudo_grad(const LrGradArgs& a, hipStream_t stream) {
  const int64_t G = lr_param_groups(a.F + 1);
  hipLaunchKernelGGL(lr_pseudo_grad_kernel, dim3((unsigned)G), dim3(kLrBlock), 0, stream, a, G);
}

}  // namespace fdx
