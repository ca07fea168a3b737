// pybind11 bindings of the linear SVC op (registered from bindings.cpp via register_svc_ops): HIP
// tensors launch the gfx950 kernel on the current stream, CPU tensors run the host twin. Shapes,
// dtypes, the scale exponents and the hot set's size (it sizes the LDS table) are validated here,
// before any launch.
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "svc.h"

namespace {

using at::Tensor;

#define FDX_CHECK(cond, msg) TORCH_CHECK(cond, "fdx.svc: ", msg)

void chk(const Tensor& t, const at::Device& dev, at::ScalarType st, const char* name) {
  FDX_CHECK(t.device() == dev, std::string(name) + " on wrong device");
  FDX_CHECK(t.is_contiguous(), std::string(name) + " must be contiguous");
  FDX_CHECK(t.scalar_type() == st, std::string(name) + " has wrong dtype");
}

double* rows_out(const c10::optional<Tensor>& t, const at::Device& dev, int64_t numel, const char* name) {
  if (!t) return nullptr;
  chk(*t, dev, at::kDouble, name);
  FDX_CHECK(t->numel() == numel, std::string(name) + " has the wrong size");
  return t->data_ptr<double>();
}

// `check_extents` reads the row pointers' extremes back (they bound what the kernel reads): a
// trainer pays that copy on its first evaluation only
void svc_eval(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& xs, double b,
              const Tensor& labels, const c10::optional<Tensor>& weights, int64_t k, int64_t kl,
              const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat, const Tensor& out,
              const c10::optional<Tensor>& margin, const c10::optional<Tensor>& r,
              const c10::optional<Tensor>& loss_row, int64_t chunk_rows, bool check_extents, int64_t threads) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the CSR's device");
  FDX_CHECK(indptr.numel() >= 1 && idx.numel() == val.numel(), "indptr holds rows + 1 entries, idx / val one per entry");
  const int64_t rows = indptr.numel() - 1;
  if (check_extents) {
    const Tensor ends = at::stack({indptr.min(), indptr.max()}).cpu();
    const int64_t* e = ends.data_ptr<int64_t>();
    if (e[0] < 0 || e[1] > idx.numel()) throw pybind11::value_error("fdx.svc: svc_eval: indptr must stay within idx");
  }
  chk(xs, dev, at::kDouble, "xs");
  FDX_CHECK(xs.dim() == 1 && xs.numel() >= 1 && xs.numel() < (int64_t(1) << 31), "xs is [F]");
  const int64_t F = xs.numel();
  chk(labels, dev, at::kDouble, "labels");
  FDX_CHECK(labels.numel() == rows, "labels needs one entry per row");
  if (weights) {
    chk(*weights, dev, at::kDouble, "weights");
    FDX_CHECK(weights->numel() == rows, "weights needs one entry per row");
  }
  FDX_CHECK(k >= 0 && k <= fdx::kNbKMax && kl >= 0 && kl <= fdx::kNbKMax, "scale exponents lie in 0 .. k_max");
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == F + 4, "out holds F + 4 sums");
  if (chunk_rows == 0) chunk_rows = fdx::kNbChunkRows;
  FDX_CHECK(chunk_rows >= 1 && chunk_rows <= fdx::kNbMaxChunkRows, "chunk_rows out of range");
  FDX_CHECK(fdx::nb_chunks(rows, chunk_rows) < (int64_t(1) << 31), "too many row chunks");
  int64_t hot_slots = 0;
  if (slot_of || hot_feat) {
    FDX_CHECK(slot_of && hot_feat, "slot_of and hot_feat come together");
    chk(*slot_of, dev, at::kShort, "slot_of");
    chk(*hot_feat, dev, at::kInt, "hot_feat");
    FDX_CHECK(slot_of->numel() == F, "slot_of needs one entry per feature");
    hot_slots = hot_feat->numel();
    FDX_CHECK(hot_slots * 8 <= fdx::kNbMaxTableBytes, "the hot set exceeds the LDS table");
  }
  double* const margin_p = rows_out(margin, dev, rows, "margin");
  double* const r_p = rows_out(r, dev, rows, "r");
  double* const loss_p = rows_out(loss_row, dev, rows, "loss_row");
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::SvcArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.xs = xs.data_ptr<double>();
    a.b = b;
    a.labels = labels.data_ptr<double>();
    a.weights = weights ? weights->data_ptr<double>() : nullptr;
    a.rows = rows;
    a.F = (int32_t)F;
    a.k = (int)k;
    a.kl = (int)kl;
    a.slot_of = hot_slots ? reinterpret_cast<const uint16_t*>(slot_of->data_ptr<int16_t>()) : nullptr;
    a.hot_feat = hot_slots ? hot_feat->data_ptr<int32_t>() : nullptr;
    a.hot_slots = (int)hot_slots;
    a.chunk_rows = (int)chunk_rows;
    a.Gq = out.data_ptr<int64_t>();
    a.gbq = a.Gq + F;
    a.lossq = a.gbq + 1;
    a.nact = a.lossq + 1;
    a.flag = a.nact + 1;
    a.margin = margin_p;
    a.r = r_p;
    a.loss_row = loss_p;
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_svc_eval<V>(a, c10::hip::getCurrentHIPStream(dev.index()).stream());
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::svc_eval_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

pybind11::dict svc_limits() {
  pybind11::dict d;
  d["chunk_rows"] = fdx::kNbChunkRows;
  d["table_bytes"] = fdx::kNbTableBytes;
  d["max_table_bytes"] = fdx::kNbMaxTableBytes;
  d["hot_slots"] = fdx::nb_hot_slots(1);
  d["max_hot_slots"] = fdx::nb_hot_slots(1, fdx::kNbMaxTableBytes);
  d["k_max"] = fdx::kNbKMax;
  d["sum_bits"] = fdx::kNbSumBits;
  d["loss_cap"] = fdx::kMlrLossCap;
  d["loss_bits"] = fdx::kMlrLossBits;
  d["flag_clamped"] = fdx::kMlrFlagClamped;
  d["flag_bad_input"] = fdx::kMlrFlagBadInput;
  d["wave"] = fdx::kNbWave;
  d["block"] = fdx::kNbBlock;
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
