// pybind11 bindings of the multinomial logistic regression op (registered from bindings.cpp via
// register_mlr_ops): HIP tensors launch the gfx950 kernel on the current stream, CPU tensors run the
// host twin. Shapes, dtypes, the class count, the scale exponents and the hot set's size (it sizes
// the LDS table) are validated here (bindings_util.h), before any launch.
#define FDX_PREFIX "fdx.mlr: "
#include "bindings_util.h"
#include "mlr.h"

namespace {

// `check_extents` reads the row pointers' extremes back (they bound what the kernel reads): a
// trainer pays that copy on its first evaluation only
void mlr_eval(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& XS, const Tensor& b,
              const Tensor& labels, const c10::optional<Tensor>& weights, int64_t k, int64_t kl,
              const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat, const Tensor& out,
              const c10::optional<Tensor>& margin, const c10::optional<Tensor>& R,
              const c10::optional<Tensor>& loss_row, int64_t chunk_rows, bool check_extents, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, check_extents);
  chk(XS, dev, at::kDouble, "XS");
  chk(b, dev, at::kDouble, "b");
  FDX_CHECK(XS.dim() == 2 && XS.size(0) >= 1 && XS.size(0) < (int64_t(1) << 31), "XS is [F, C]");
  const int64_t F = XS.size(0), C = XS.size(1);
  chk_classes(C);
  FDX_CHECK(b.numel() == C, "b is [C]");
  chk_row_labels(labels, weights, dev, rows);
  chk_scale_exponents(k, kl);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == F * C + C + 2, "out holds F C + C + 2 sums");
  chunk_rows = chunk_rows_or_default(chunk_rows, rows);
  const int64_t hot_slots = chk_hot_set(slot_of, hot_feat, dev, F, C);
  double* const margin_p = rows_out(margin, dev, rows * C, "margin");
  double* const R_p = rows_out(R, dev, rows * C, "R");
  double* const loss_p = rows_out(loss_row, dev, rows, "loss_row");
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::MlrArgs<V> a{};
    fill_csr_rows<V>(a, indptr, idx, val, labels, weights, F);
    fill_hot_set(a, slot_of, hot_feat, hot_slots, chunk_rows);
    a.XS = XS.data_ptr<double>();
    a.b = b.data_ptr<double>();
    a.num_classes = (int)C;
    a.k = (int)k;
    a.kl = (int)kl;
    a.Gq = out.data_ptr<int64_t>();
    a.gbq = a.Gq + F * C;
    a.lossq = a.gbq + C;
    a.flag = a.lossq + 1;
    a.margin = margin_p;
    a.R = R_p;
    a.loss_row = loss_p;
    run_on(dev, [&](hipStream_t s) { fdx::launch_mlr_eval<V>(a, s); }, [&] { fdx::mlr_eval_cpu<V>(a, (int)threads); });
  });
}

pybind11::dict mlr_limits() {
  pybind11::dict d = pass_limits(true);
  d["max_classes"] = fdx::kNbMaxClasses;
  return d;
}

}  // namespace

void register_mlr_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("mlr_eval", &mlr_eval,
        "one evaluation of multinomial logistic regression over a CSR (Gq, gbq, lossq, flag in one int64 block)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("XS"), py::arg("b"), py::arg("labels"),
        py::arg("weights"), py::arg("k"), py::arg("kl"), py::arg("slot_of"), py::arg("hot_feat"), py::arg("out"),
        py::arg("margin") = py::none(), py::arg("R") = py::none(), py::arg("loss_row") = py::none(),
        py::arg("chunk_rows") = 0, py::arg("check_extents") = true, py::arg("threads") = 0);
  m.def("mlr_limits", &mlr_limits, "structural constants of the multinomial logistic regression kernel");
}
