// pybind11 bindings of the multi-class boosting ops (registered from bindings.cpp via
// register_softprob_ops): HIP tensors launch the gfx950 kernels on the current stream, CPU tensors
// run the host twins. Shapes, dtypes, strides and the class count are validated here, before any
// launch; class ids and tree features are validated by ops/sparse.py on the host arrays.
#define FDX_PREFIX "fdx.softprob: "
#include "bindings_util.h"

#include "softprob.h"

namespace {

void check_classes(int64_t C) {
  if (C < 2 || C > fdx::kSoftprobMaxClasses)
    throw pybind11::value_error("fdx.softprob: the class count must lie in 2 .. max_classes");
}

// C planes of N rows: rows contiguous, planes a non-negative stride >= N apart (a view of a wider buffer)
int64_t planes(const Tensor& t, const at::Device& dev, at::ScalarType st, int64_t C, int64_t N, const char* name) {
  FDX_CHECK(t.device() == dev, std::string(name) + " on wrong device");
  FDX_CHECK(t.scalar_type() == st, std::string(name) + " has wrong dtype");
  FDX_CHECK(t.dim() == 2 && t.size(0) == C && t.size(1) == N, std::string(name) + " is [C, N]");
  FDX_CHECK(N <= 1 || t.stride(1) == 1, std::string(name) + ": the rows of a plane must be contiguous");
  FDX_CHECK(t.stride(0) >= N, std::string(name) + ": planes overlap");
  return t.stride(0);
}

void softprob_grad(const Tensor& margin, const Tensor& y, const c10::optional<Tensor>& w, const Tensor& g,
                   const Tensor& h, int64_t threads) {
  const auto dev = margin.device();
  FDX_CHECK(margin.dim() == 2, "margin is [C, N]");
  const int64_t C = margin.size(0), N = margin.size(1);
  check_classes(C);
  fdx::SoftprobGradArgs a{};
  a.margin_stride = planes(margin, dev, at::kDouble, C, N, "margin");
  a.g_stride = planes(g, dev, at::kFloat, C, N, "g");
  a.h_stride = planes(h, dev, at::kFloat, C, N, "h");
  chk(y, dev, at::kFloat, "y");
  FDX_CHECK(y.numel() == N, "y needs one entry per row");
  if (w) {
    chk(*w, dev, at::kFloat, "w");
    FDX_CHECK(w->numel() == N, "w needs one entry per row");
  }
  if (N == 0) return;
  a.margin = margin.data_ptr<double>();
  a.y = y.data_ptr<float>();
  a.w = w ? w->data_ptr<float>() : nullptr;
  a.g = g.data_ptr<float>();
  a.h = h.data_ptr<float>();
  a.N = N;
  a.num_classes = (int)C;
  FDX_CHECK((N + fdx::kSoftprobBlock - 1) / fdx::kSoftprobBlock < (int64_t(1) << 31), "too many rows for one launch");
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_softprob_grad(a, c10::hip::getCurrentHIPStream(dev.index()).stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::softprob_grad_cpu(a, (int)threads);
  }
}

// trees = (feat, thr, left, right, leaf, roots), leaf scalar per node
void score_class_trees(const Tensor& indptr, const Tensor& idx, const Tensor& val, const std::vector<Tensor>& trees,
                       const Tensor& tree_class, int64_t num_classes, bool cmp_less, const Tensor& out,
                       int64_t threads) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the CSR's device");
  FDX_CHECK(indptr.numel() >= 1 && idx.numel() == val.numel(), "indptr holds rows + 1 entries, idx / val one per entry");
  const int64_t rows = indptr.numel() - 1;
  check_classes(num_classes);
  FDX_CHECK(trees.size() == 6, "trees = (feat, thr, left, right, leaf, roots)");
  const at::ScalarType want[6] = {at::kInt, at::kDouble, at::kInt, at::kInt, at::kDouble, at::kInt};
  for (int i = 0; i < 6; ++i) chk(trees[i], dev, want[i], "tree arrays");
  const int64_t nodes = trees[0].numel();
  FDX_CHECK(nodes >= 1 && nodes < (int64_t(1) << 31), "a tree list has at least one node");
  for (int i = 1; i < 5; ++i) FDX_CHECK(trees[i].numel() == nodes, "node arrays: one entry per node");
  chk(tree_class, dev, at::kInt, "tree_class");
  FDX_CHECK(tree_class.numel() == trees[5].numel(), "tree_class needs one entry per tree");
  chk(out, dev, at::kDouble, "out");
  FDX_CHECK(out.numel() == rows * num_classes, "out is [rows, C]");
  FDX_CHECK((rows + 3) / 4 < (int64_t(1) << 31), "too many rows for one launch");
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::ClassTreeArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.rows = rows;
    a.trees.feat = trees[0].data_ptr<int32_t>();
    a.trees.thr = trees[1].data_ptr<double>();
    a.trees.left = trees[2].data_ptr<int32_t>();
    a.trees.right = trees[3].data_ptr<int32_t>();
    a.trees.leaf = trees[4].data_ptr<double>();
    a.trees.roots = trees[5].data_ptr<int32_t>();
    a.trees.weights = nullptr;
    a.trees.num_trees = (int32_t)trees[5].numel();
    a.trees.K = 1;
    a.tree_class = tree_class.data_ptr<int32_t>();
    a.num_classes = (int)num_classes;
    a.cmp_less = cmp_less;
    a.out = out.data_ptr<double>();
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_score_class_trees<V>(a, c10::hip::getCurrentHIPStream(dev.index()).stream());
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::score_class_trees_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

pybind11::dict softprob_limits() {
  pybind11::dict d;
  d["max_classes"] = fdx::kSoftprobMaxClasses;
  d["block"] = fdx::kSoftprobBlock;
  d["wave"] = fdx::kSoftprobWave;
  d["min_hess"] = fdx::kSoftprobMinHess;
  return d;
}

}  // namespace

void register_softprob_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("softprob_grad", &softprob_grad, "the 2 C gradient planes of multi:softprob from the C margin planes",
        py::arg("margin"), py::arg("y"), py::arg("w"), py::arg("g"), py::arg("h"), py::arg("threads") = 0);
  m.def("score_class_trees", &score_class_trees, "class-grouped tree-ensemble scoring of a CSR feature matrix",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("trees"), py::arg("tree_class"),
        py::arg("num_classes"), py::arg("cmp_less"), py::arg("out"), py::arg("threads") = 0);
  m.def("softprob_limits", &softprob_limits, "structural constants of the multi-class boosting kernels");
}
