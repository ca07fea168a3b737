// pybind11 bindings of the linear SVC op (registered from bindings.cpp via register_svc_ops): HIP
// tensors launch the gfx950 kernel on the current stream, CPU tensors run the host twin. Shapes,
// dtypes, the scale exponents and the hot set's size (it sizes the LDS table) are validated here
// (bindings_util.h), before any launch.
#define FDX_PREFIX "fdx.svc: "
#include "bindings_util.h"
#include "svc.h"

namespace {

// `check_extents` reads the row pointers' extremes back (they bound what the kernel reads): a
// trainer pays that copy on its first evaluation only
void svc_eval(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& xs, double b,
              const Tensor& labels, const c10::optional<Tensor>& weights, int64_t k, int64_t kl,
              const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat, const Tensor& out,
              const c10::optional<Tensor>& margin, const c10::optional<Tensor>& r,
              const c10::optional<Tensor>& loss_row, int64_t chunk_rows, bool check_extents, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, check_extents, "svc_eval");
  chk(xs, dev, at::kDouble, "xs");
  FDX_CHECK(xs.dim() == 1 && xs.numel() >= 1 && xs.numel() < (int64_t(1) << 31), "xs is [F]");
  const int64_t F = xs.numel();
  chk_row_labels(labels, weights, dev, rows);
  chk_scale_exponents(k, kl);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == F + 4, "out holds F + 4 sums");
  chunk_rows = chunk_rows_or_default(chunk_rows, rows);
  const int64_t hot_slots = chk_hot_set(slot_of, hot_feat, dev, F, 1);
  double* const margin_p = rows_out(margin, dev, rows, "margin");
  double* const r_p = rows_out(r, dev, rows, "r");
  double* const loss_p = rows_out(loss_row, dev, rows, "loss_row");
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::SvcArgs<V> a{};
    fill_csr_rows<V>(a, indptr, idx, val, labels, weights, F);
    fill_hot_set(a, slot_of, hot_feat, hot_slots, chunk_rows);
    a.xs = xs.data_ptr<double>();
    a.b = b;
    a.k = (int)k;
    a.kl = (int)kl;
    a.Gq = out.data_ptr<int64_t>();
    a.gbq = a.Gq + F;
    a.lossq = a.gbq + 1;
    a.nact = a.lossq + 1;
    a.flag = a.nact + 1;
    a.margin = margin_p;
    a.r = r_p;
    a.loss_row = loss_p;
    run_on(dev, [&](hipStream_t s) { fdx::launch_svc_eval<V>(a, s); }, [&] { fdx::svc_eval_cpu<V>(a, (int)threads); });
  });
}

pybind11::dict svc_limits() {
  pybind11::dict d = pass_limits(true);
  d["hot_slots"] = fdx::nb_hot_slots(1);
  d["max_hot_slots"] = fdx::nb_hot_slots(1, fdx::kNbMaxTableBytes);
  return d;
}

}  // namespace

void register_svc_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("svc_eval", &svc_eval,
        "one evaluation of the linear SVC hinge objective over a CSR (Gq, gbq, lossq, nact, flag in one int64 block)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("xs"), py::arg("b"), py::arg("labels"),
        py::arg("weights"), py::arg("k"), py::arg("kl"), py::arg("slot_of"), py::arg("hot_feat"), py::arg("out"),
        py::arg("margin") = py::none(), py::arg("r") = py::none(), py::arg("loss_row") = py::none(),
        py::arg("chunk_rows") = 0, py::arg("check_extents") = true, py::arg("threads") = 0);
  m.def("svc_limits", &svc_limits, "structural constants of the linear SVC kernel");
}
