// pybind11 bindings of the Naive Bayes ops (registered from bindings.cpp via register_nb_ops): HIP
// tensors launch the gfx950 kernels on the current stream, CPU tensors run the host twins. Shapes,
// dtypes, the class count, the scale exponents and the hot set's size (it sizes the LDS table) are
// validated here (bindings_util.h), before any launch.
#define FDX_PREFIX "fdx.nb: "
#include "bindings_util.h"
#include "nb.h"

namespace {

void nb_sums(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& labels,
             const c10::optional<Tensor>& weights, int64_t num_classes, int64_t num_features, int64_t k, int64_t kw,
             bool bernoulli, const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat,
             const Tensor& out, int64_t chunk_rows, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, true);
  chk_row_labels(labels, weights, dev, rows);
  chk_classes(num_classes);
  FDX_CHECK(num_features >= 1 && num_features < (int64_t(1) << 31), "num_features out of range");
  chk_scale_exponents(k, kw);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == num_classes * num_features + 2 * num_classes + 1, "out holds C F + 2 C + 1 sums");
  chunk_rows = chunk_rows_or_default(chunk_rows, rows);
  const int64_t hot_slots = chk_hot_set(slot_of, hot_feat, dev, num_features, num_classes);
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::NbSumArgs<V> a{};
    fill_csr_rows<V>(a, indptr, idx, val, labels, weights, num_features);
    fill_hot_set(a, slot_of, hot_feat, hot_slots, chunk_rows);
    a.num_classes = (int)num_classes;
    a.k = (int)k;
    a.kw = (int)kw;
    a.bernoulli = bernoulli;
    a.S = out.data_ptr<int64_t>();
    a.Wq = a.S + num_classes * num_features;
    a.cnt = a.Wq + num_classes;
    a.flag = a.cnt + num_classes;
    run_on(dev, [&](hipStream_t s) { fdx::launch_nb_sums<V>(a, s); }, [&] { fdx::nb_sums_cpu<V>(a, (int)threads); });
  });
}

void nb_score(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& W, const Tensor& b,
              const Tensor& out, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, false);
  chk(W, dev, at::kDouble, "W");
  chk(b, dev, at::kDouble, "b");
  chk(out, dev, at::kDouble, "out");
  FDX_CHECK(W.dim() == 2 && W.size(0) >= 1 && W.size(0) < (int64_t(1) << 31), "W is [F, C]");
  const int64_t C = W.size(1);
  chk_classes(C);
  FDX_CHECK(b.numel() == C && out.numel() == rows * C, "b [C], out [rows, C]");
  FDX_CHECK((rows + fdx::kNbWaves - 1) / fdx::kNbWaves < (int64_t(1) << 31), "too many rows");
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::NbScoreArgs<V> a{indptr.data_ptr<int64_t>(), idx.data_ptr<int32_t>(), val.data_ptr<V>(), rows,
                          (int32_t)W.size(0), (int)C, W.data_ptr<double>(), b.data_ptr<double>(),
                          out.data_ptr<double>()};
    run_on(dev, [&](hipStream_t s) { fdx::launch_nb_score<V>(a, s); }, [&] { fdx::nb_score_cpu<V>(a, (int)threads); });
  });
}

pybind11::dict nb_limits() {
  pybind11::dict d = pass_limits(false);
  d["max_classes"] = fdx::kNbMaxClasses;
  d["prefix_rows"] = fdx::kNbPrefixRows;
  return d;
}

}  // namespace

void register_nb_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("nb_sums", &nb_sums, "exact fixed-point class-conditional sums of a CSR (S, Wq, cnt, flag in one int64 block)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("labels"), py::arg("weights"),
        py::arg("num_classes"), py::arg("num_features"), py::arg("k"), py::arg("kw"), py::arg("bernoulli"),
        py::arg("slot_of"), py::arg("hot_feat"), py::arg("out"), py::arg("chunk_rows") = 0, py::arg("threads") = 0);
  m.def("nb_score", &nb_score, "raw[r, c] = b_c + X W[:, c] in spmv's order", py::arg("indptr"), py::arg("idx"),
        py::arg("val"), py::arg("W"), py::arg("b"), py::arg("out"), py::arg("threads") = 0);
  m.def("nb_limits", &nb_limits, "structural constants of the Naive Bayes kernels");
}
