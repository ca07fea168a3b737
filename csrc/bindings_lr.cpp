// pybind11 bindings of the elastic-net logistic-regression ops (registered from bindings.cpp via
// register_lr_ops): HIP tensors launch the gfx950 kernels on the current stream, CPU tensors run
// the host twins. Shapes, dtypes and the 16-byte alignment the parameter passes load with are
// validated here, before any launch.
#define FDX_PREFIX "fdx.lr: "
#include "bindings_util.h"

#include "lr.h"
#include "ops.h"

namespace {

using c10::optional;

void chk16(const Tensor& t, const char* name) {
  FDX_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, std::string(name) + " must be 16-byte aligned");
}

// partials: [2, ceil(rows / rows_per_partial)] (sum w loss, sum r)
void lr_forward(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& xs, const Tensor& b,
                const Tensor& y, const Tensor& w, const Tensor& r, const optional<Tensor>& loss_row,
                const optional<Tensor>& margin, const Tensor& partials, int64_t threads) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the CSR's device");
  chk(xs, dev, at::kDouble, "xs");
  chk(b, dev, at::kDouble, "b");
  chk(y, dev, at::kDouble, "y");
  chk(w, dev, at::kDouble, "w");
  chk(r, dev, at::kDouble, "r");
  chk(partials, dev, at::kDouble, "partials");
  const int64_t rows = indptr.numel() - 1;
  FDX_CHECK(rows >= 0 && rows / fdx::kLrRowsPerPartial < (int64_t)INT32_MAX, "row count out of range");
  FDX_CHECK(idx.numel() == val.numel(), "idx / val size");
  FDX_CHECK(b.numel() == 1, "b holds one value");
  FDX_CHECK(y.numel() == rows && w.numel() == rows && r.numel() == rows, "y, w, r need one entry per row");
  FDX_CHECK(partials.numel() == 2 * fdx::lr_forward_partials(rows), "partials [2, ceil(rows / rows_per_partial)]");
  auto opt = [&](const optional<Tensor>& t, const char* name) -> double* {
    if (!t || !t->defined()) return nullptr;
    chk(*t, dev, at::kDouble, name);
    FDX_CHECK(t->numel() == rows, std::string(name) + " needs one entry per row");
    return t->data_ptr<double>();
  };
  double* lp = opt(loss_row, "loss_row");
  double* mp = opt(margin, "margin");
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::LrForwardArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.rows = rows;
    a.xs = xs.data_ptr<double>();
    a.b = b.data_ptr<double>();
    a.y = y.data_ptr<double>();
    a.w = w.data_ptr<double>();
    a.r = r.data_ptr<double>();
    a.loss_row = lp;
    a.margin = mp;
    a.partials = partials.data_ptr<double>();
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_lr_forward<V>(a, stream(dev));
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::lr_forward_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

// out[k] = sum of partials[k, :] in the reducer's fixed order
void lr_reduce(const Tensor& partials, const Tensor& out) {
  const auto dev = partials.device();
  chk(partials, dev, at::kDouble, "partials");
  chk(out, dev, at::kDouble, "out");
  FDX_CHECK(partials.dim() == 2 && out.numel() == partials.size(0), "partials [K, P], out [K]");
  fdx::LrReduceArgs a{partials.data_ptr<double>(), partials.size(0), partials.size(1), out.data_ptr<double>()};
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_lr_reduce(a, stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::lr_reduce_cpu(a);
  }
}

void lr_owlqn_step(const Tensor& x, const Tensor& d, const Tensor& xi, const Tensor& pg, const Tensor& scale, double t,
                   const Tensor& x_new, const Tensor& xs_new, const Tensor& partials, int64_t threads) {
  const auto dev = x.device();
  const int64_t n = x.numel(), F = n - 1;
  FDX_CHECK(n >= 1, "x holds F coefficients and the intercept");
  const Tensor* full[] = {&x, &d, &xi, &pg, &x_new};
  const char* names[] = {"x", "d", "xi", "pg", "x_new"};
  for (int i = 0; i < 5; ++i) {
    chk(*full[i], dev, at::kDouble, names[i]);
    chk16(*full[i], names[i]);
    FDX_CHECK(full[i]->numel() == n, std::string(names[i]) + " needs F + 1 entries");
  }
  chk(scale, dev, at::kDouble, "scale");
  chk(xs_new, dev, at::kDouble, "xs_new");
  chk(partials, dev, at::kDouble, "partials");
  chk16(scale, "scale");
  chk16(xs_new, "xs_new");
  FDX_CHECK(scale.numel() == F && xs_new.numel() == F, "scale, xs_new need F entries");
  FDX_CHECK(partials.numel() == 3 * fdx::lr_param_groups(n), "partials [3, lr_param_groups(F + 1)]");
  fdx::LrStepArgs a{};
  a.x = x.data_ptr<double>();
  a.d = d.data_ptr<double>();
  a.xi = xi.data_ptr<double>();
  a.pg = pg.data_ptr<double>();
  a.scale = scale.data_ptr<double>();
  a.t = t;
  a.F = F;
  a.x_new = x_new.data_ptr<double>();
  a.xs_new = xs_new.data_ptr<double>();
  a.partials = partials.data_ptr<double>();
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_lr_owlqn_step(a, stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::lr_owlqn_step_cpu(a, (int)threads);
  }
}

// parts: [F + 2] = (sum w loss, sum r, X^T r)
void lr_pseudo_grad(const Tensor& parts, const Tensor& scale, const Tensor& x, double W, double l1, double l2,
                    bool fit_intercept, const Tensor& g, const Tensor& pg, const Tensor& xi, const Tensor& partials,
                    int64_t threads) {
  const auto dev = x.device();
  const int64_t n = x.numel(), F = n - 1;
  FDX_CHECK(n >= 1, "x holds F coefficients and the intercept");
  const Tensor* full[] = {&x, &g, &pg, &xi};
  const char* names[] = {"x", "g", "pg", "xi"};
  for (int i = 0; i < 4; ++i) {
    chk(*full[i], dev, at::kDouble, names[i]);
    chk16(*full[i], names[i]);
    FDX_CHECK(full[i]->numel() == n, std::string(names[i]) + " needs F + 1 entries");
  }
  chk(parts, dev, at::kDouble, "parts");
  chk(scale, dev, at::kDouble, "scale");
  chk(partials, dev, at::kDouble, "partials");
  chk16(parts, "parts");
  chk16(scale, "scale");
  FDX_CHECK(parts.numel() == F + 2 && scale.numel() == F, "parts [F + 2], scale [F]");
  FDX_CHECK(partials.numel() == fdx::lr_param_groups(n), "partials [lr_param_groups(F + 1)]");
  FDX_CHECK(W > 0.0 && l1 >= 0.0 && l2 >= 0.0, "W > 0, l1 >= 0, l2 >= 0");
  fdx::LrGradArgs a{};
  a.parts = parts.data_ptr<double>();
  a.scale = scale.data_ptr<double>();
  a.x = x.data_ptr<double>();
  a.W = W;
  a.l1 = l1;
  a.l2 = l2;
  a.F = F;
  a.fit_intercept = fit_intercept;
  a.g = g.data_ptr<double>();
  a.pg = pg.data_ptr<double>();
  a.xi = xi.data_ptr<double>();
  a.partials = partials.data_ptr<double>();
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_lr_pseudo_grad(a, stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::lr_pseudo_grad_cpu(a, (int)threads);
  }
}

int64_t lr_param_groups(int64_t n) { return fdx::lr_param_groups(n); }

pybind11::dict lr_limits() {
  pybind11::dict d;
  d["rows_per_partial"] = fdx::kLrRowsPerPartial;
  d["reduce_block"] = fdx::kLrReduceBlock;
  d["block"] = fdx::kLrBlock;
  d["max_groups"] = fdx::kLrMaxGroups;   // beyond 2 * block * max_groups parameters the lanes loop
  return d;
}

}  // namespace

void register_lr_ops(pybind11::module& m) {
  m.def("lr_forward", &lr_forward, "fused margin / log-loss / residual of a CSR with per-workgroup partials");
  m.def("lr_reduce", &lr_reduce, "fixed-order sums of rows of partials (one workgroup)");
  m.def("lr_owlqn_step", &lr_owlqn_step, "projected OWL-QN trial point with partials of its norms and decrease");
  m.def("lr_pseudo_grad", &lr_pseudo_grad, "smooth gradient, pseudo-gradient and orthant with partials of |pg|^2");
  m.def("lr_param_groups", &lr_param_groups, "workgroups (partials) of a pass over n parameters");
  m.def("lr_limits", &lr_limits, "structural constants of the logistic-regression kernels");
}
