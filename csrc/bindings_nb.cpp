// pybind11 bindings of the Naive Bayes ops (registered from bindings.cpp via register_nb_ops): HIP
// tensors launch the gfx950 kernels on the current stream, CPU tensors run the host twins. Shapes,
// dtypes, the class count, the scale exponents and the hot set's size (it sizes the LDS table) are
// validated here, before any launch.
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "nb.h"

namespace {

using at::Tensor;

#define FDX_CHECK(cond, msg) TORCH_CHECK(cond, "fdx.nb: ", msg)

void chk(const Tensor& t, const at::Device& dev, at::ScalarType st, const char* name) {
  FDX_CHECK(t.device() == dev, std::string(name) + " on wrong device");
  FDX_CHECK(t.is_contiguous(), std::string(name) + " must be contiguous");
  FDX_CHECK(t.scalar_type() == st, std::string(name) + " has wrong dtype");
}

// dtypes and sizes of a CSR; with `extents` the row pointers are read back too (they bound what the
// kernels read): the fit pass pays one small copy, the scorer trusts its column as spmv does
int64_t chk_csr(const Tensor& indptr, const Tensor& idx, const Tensor& val, bool extents) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the CSR's device");
  FDX_CHECK(indptr.numel() >= 1 && idx.numel() == val.numel(), "indptr holds rows + 1 entries, idx / val one per entry");
  if (extents) {
    const Tensor ends = at::stack({indptr.min(), indptr.max()}).cpu();
    const int64_t* e = ends.data_ptr<int64_t>();
    FDX_CHECK(e[0] >= 0 && e[1] <= idx.numel(), "indptr must stay within idx");
  }
  return indptr.numel() - 1;
}

hipStream_t stream(const at::Device& d) { return c10::hip::getCurrentHIPStream(d.index()).stream(); }

void nb_sums(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& labels,
             const c10::optional<Tensor>& weights, int64_t num_classes, int64_t num_features, int64_t k, int64_t kw,
             bool bernoulli, const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat,
             const Tensor& out, int64_t chunk_rows, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, true);
  chk(labels, dev, at::kDouble, "labels");
  FDX_CHECK(labels.numel() == rows, "labels needs one entry per row");
  if (weights) {
    chk(*weights, dev, at::kDouble, "weights");
    FDX_CHECK(weights->numel() == rows, "weights needs one entry per row");
  }
  if (num_classes < 2 || num_classes > fdx::kNbMaxClasses)
    throw pybind11::value_error("fdx.nb: the class count must lie in 2 .. max_classes");
  FDX_CHECK(num_features >= 1 && num_features < (int64_t(1) << 31), "num_features out of range");
  FDX_CHECK(k >= 0 && k <= fdx::kNbKMax && kw >= 0 && kw <= fdx::kNbKMax, "scale exponents lie in 0 .. k_max");
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == num_classes * num_features + 2 * num_classes + 1, "out holds C F + 2 C + 1 sums");
  if (chunk_rows == 0) chunk_rows = fdx::kNbChunkRows;
  FDX_CHECK(chunk_rows >= 1 && chunk_rows <= fdx::kNbMaxChunkRows, "chunk_rows out of range");
  FDX_CHECK(fdx::nb_chunks(rows, chunk_rows) < (int64_t(1) << 31), "too many row chunks");
  int64_t hot_slots = 0;
  if (slot_of || hot_feat) {
    FDX_CHECK(slot_of && hot_feat, "slot_of and hot_feat come together");
    chk(*slot_of, dev, at::kShort, "slot_of");
    chk(*hot_feat, dev, at::kInt, "hot_feat");
    FDX_CHECK(slot_of->numel() == num_features, "slot_of needs one entry per feature");
    hot_slots = hot_feat->numel();
    FDX_CHECK(num_classes * hot_slots * 8 <= fdx::kNbMaxTableBytes, "the hot set exceeds the LDS table");
  }
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::NbSumArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.labels = labels.data_ptr<double>();
    a.weights = weights ? weights->data_ptr<double>() : nullptr;
    a.rows = rows;
    a.F = (int32_t)num_features;
    a.num_classes = (int)num_classes;
    a.k = (int)k;
    a.kw = (int)kw;
    a.bernoulli = bernoulli;
    a.slot_of = hot_slots ? reinterpret_cast<const uint16_t*>(slot_of->data_ptr<int16_t>()) : nullptr;
    a.hot_feat = hot_slots ? hot_feat->data_ptr<int32_t>() : nullptr;
    a.hot_slots = (int)hot_slots;
    a.chunk_rows = (int)chunk_rows;
    a.S = out.data_ptr<int64_t>();
    a.Wq = a.S + num_classes * num_features;
    a.cnt = a.Wq + num_classes;
    a.flag = a.cnt + num_classes;
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_nb_sums<V>(a, stream(dev));
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::nb_sums_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
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
  if (C < 2 || C > fdx::kNbMaxClasses) throw pybind11::value_error("fdx.nb: the class count must lie in 2 .. max_classes");
  FDX_CHECK(b.numel() == C && out.numel() == rows * C, "b [C], out [rows, C]");
  FDX_CHECK((rows + fdx::kNbWaves - 1) / fdx::kNbWaves < (int64_t(1) << 31), "too many rows");
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::NbScoreArgs<V> a{indptr.data_ptr<int64_t>(), idx.data_ptr<int32_t>(), val.data_ptr<V>(), rows,
                          (int32_t)W.size(0), (int)C, W.data_ptr<double>(), b.data_ptr<double>(),
                          out.data_ptr<double>()};
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_nb_score<V>(a, stream(dev));
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::nb_score_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

pybind11::dict nb_limits() {
  pybind11::dict d;
  d["max_classes"] = fdx::kNbMaxClasses;
  d["chunk_rows"] = fdx::kNbChunkRows;
  d["table_bytes"] = fdx::kNbTableBytes;
  d["max_table_bytes"] = fdx::kNbMaxTableBytes;
  d["k_max"] = fdx::kNbKMax;
  d["sum_bits"] = fdx::kNbSumBits;
  d["prefix_rows"] = fdx::kNbPrefixRows;
  d["wave"] = fdx::kNbWave;
  d["block"] = fdx::kNbBlock;
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
