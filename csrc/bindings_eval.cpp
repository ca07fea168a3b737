// pybind11 bindings of the validation-monitoring ops (registered from bindings.cpp via
// register_eval_ops): HIP tensors launch the gfx950 kernels on the current stream, CPU tensors
// run the host twins. Shapes are validated here, before any launch.
#define FDX_PREFIX "fdx.eval: "
#include "bindings_util.h"

#include "eval.h"
#include "ops.h"

namespace {

using c10::optional;

// table: (feat, bin, left, right, leaf, stats, kexp) of the level loop's node table;
// quant: (fid_orig, boff, thresholds) of the Quantized features
void tree_eval_update(const Tensor& indptr, const Tensor& idx, const Tensor& val, const std::vector<Tensor>& table,
                      const std::vector<Tensor>& quant, double eta, double lambda, double mds, const Tensor& margin,
                      int64_t threads) {
  const auto dev = margin.device();
  chk(margin, dev, at::kDouble, "margin");
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the margin's device");
  const int64_t rows = margin.numel();
  FDX_CHECK(indptr.numel() == rows + 1, "indptr needs rows + 1 entries");
  FDX_CHECK(idx.numel() == val.numel(), "idx / val size");
  FDX_CHECK(table.size() == 7, "table = (feat, bin, left, right, leaf, stats, kexp)");
  FDX_CHECK(quant.size() == 3, "quant = (fid_orig, boff, thresholds)");
  for (int i = 0; i < 4; ++i) chk(table[i], dev, at::kInt, "node table");
  chk(table[4], dev, at::kByte, "leaf");
  chk(table[5], dev, at::kLong, "stats");
  chk(table[6], dev, at::kInt, "kexp");
  chk(quant[0], dev, at::kLong, "fid_orig");
  chk(quant[1], dev, at::kLong, "boff");
  chk(quant[2], dev, at::kDouble, "thresholds");
  const int64_t M = table[0].numel();
  FDX_CHECK(M >= 1 && M <= fdx::kEvalMaxNodes, "node table size");
  for (int i = 1; i < 5; ++i) FDX_CHECK(table[i].numel() == M, "node table arrays size");
  FDX_CHECK(table[5].numel() == 2 * M && table[6].numel() == 2, "stats [M, 2], kexp [2]");
  FDX_CHECK(quant[1].numel() == quant[0].numel() + 1, "boff needs Fa + 1 entries");
  fdx::EvalTree t{};
  t.feat = table[0].data_ptr<int32_t>();
  t.bin = table[1].data_ptr<int32_t>();
  t.left = table[2].data_ptr<int32_t>();
  t.right = table[3].data_ptr<int32_t>();
  t.leaf = table[4].data_ptr<uint8_t>();
  t.stats = table[5].data_ptr<int64_t>();
  t.kexp = table[6].data_ptr<int32_t>();
  t.fid_orig = quant[0].data_ptr<int64_t>();
  t.boff = quant[1].data_ptr<int64_t>();
  t.thresholds = quant[2].data_ptr<double>();
  t.max_nodes = (int32_t)M;
  t.Fa = quant[0].numel();
  t.TB = quant[2].numel();
  t.eta = eta;
  t.lambda = lambda;
  t.mds = mds;
  auto run = [&](auto tag) {
    using V = decltype(tag);
    fdx::TreeEvalArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.rows = rows;
    a.t = t;
    a.margin = margin.data_ptr<double>();
    if (dev.is_cuda()) {
      c10::hip::HIPGuard guard(dev.index());
      fdx::launch_tree_eval_update<V>(a, stream(dev));
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      fdx::tree_eval_update_cpu<V>(a, (int)threads);
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

// out[0..3) += (logloss, error, weight) sums in 2^-k units (zeroed by the caller)
void eval_sums(const Tensor& margin, const Tensor& label, const optional<Tensor>& weight, int64_t k, const Tensor& out,
               int64_t blocks, int64_t threads) {
  const auto dev = margin.device();
  chk(margin, dev, at::kDouble, "margin");
  chk(label, dev, at::kFloat, "label");
  chk(out, dev, at::kLong, "out");
  const int64_t n = margin.numel();
  FDX_CHECK(label.numel() == n && out.numel() == 3, "label [n], out [3]");
  FDX_CHECK(k >= 0 && k <= 40, "fixed-point exponent out of range");
  fdx::EvalSumArgs a{};
  a.margin = margin.data_ptr<double>();
  a.label = label.data_ptr<float>();
  a.weight = nullptr;
  if (weight && weight->defined()) {
    chk(*weight, dev, at::kFloat, "weight");
    FDX_CHECK(weight->numel() == n, "weight size");
    a.weight = weight->data_ptr<float>();
  }
  a.n = n;
  a.scale = ldexp(1.0, (int)k);
  a.out = out.data_ptr<int64_t>();
  if (dev.is_cuda()) {
    FDX_CHECK(blocks <= 65536, "too many workgroups");
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_eval_sums(a, (int)blocks, stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::eval_sums_cpu(a, (int)threads);
  }
}

// out = (U2, P, N); device scratch (key / label double buffers, tiles, hipCUB temporary) comes from
// the caching allocator on the current stream
void eval_auc(const Tensor& margin, const Tensor& label, const Tensor& out) {
  const auto dev = margin.device();
  chk(margin, dev, at::kDouble, "margin");
  chk(label, dev, at::kFloat, "label");
  chk(out, dev, at::kLong, "out");
  const int64_t n = margin.numel();
  FDX_CHECK(label.numel() == n && out.numel() == 3, "label [n], out [3]");
  if (!dev.is_cuda()) {
    fdx::eval_auc_cpu(margin.data_ptr<double>(), label.data_ptr<float>(), n, out.data_ptr<int64_t>());
    return;
  }
  c10::hip::HIPGuard guard(dev.index());
  const int64_t cap = n > 0 ? n : 1;
  const auto o64 = at::TensorOptions().device(dev).dtype(at::kLong);
  const auto o8 = at::TensorOptions().device(dev).dtype(at::kByte);
  Tensor keys = at::empty({2 * cap}, o64);
  Tensor labels = at::empty({2 * cap}, o8);
  Tensor tiles = at::empty({4 * fdx::eval_auc_tiles(n)}, o64);
  fdx::EvalAucScratch s{};
  s.temp_bytes = fdx::eval_auc_temp_bytes(n);
  Tensor temp = at::empty({(int64_t)s.temp_bytes + 8}, o8);
  s.keys[0] = reinterpret_cast<uint64_t*>(keys.data_ptr<int64_t>());
  s.keys[1] = s.keys[0] + cap;
  s.labels[0] = labels.data_ptr<uint8_t>();
  s.labels[1] = s.labels[0] + cap;
  s.temp = temp.data_ptr<uint8_t>();
  s.tiles = tiles.data_ptr<int64_t>();
  fdx::launch_eval_auc(margin.data_ptr<double>(), label.data_ptr<float>(), n, s, out.data_ptr<int64_t>(), stream(dev));
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

int64_t eval_sum_kexp(int64_t n_global, double w_max) { return fdx::eval_sum_kexp(n_global, w_max); }

pybind11::dict eval_limits() {
  pybind11::dict d;
  d["rows_per_group"] = fdx::kEvalRowsPerGroup;
  d["max_groups"] = fdx::kEvalMaxGroups;   // beyond rows_per_group * max_groups rows the waves loop
  d["wave_load"] = fdx::kEvalWaveLoad;
  d["auc_tile"] = fdx::kEvalAucTile;
  d["reduce_block"] = fdx::kEvalReduceBlock;
  return d;
}

}  // namespace

void register_eval_ops(pybind11::module& m) {
  m.def("tree_eval_update", &tree_eval_update, "val_margin += leaf values of a raw-valued CSR in the device node table");
  m.def("eval_sums", &eval_sums, "exact fixed-point logloss / error / weight sums");
  m.def("eval_auc", &eval_auc, "exact tie-aware AUC integers (U2, P, N)");
  m.def("eval_sum_kexp", &eval_sum_kexp, "fixed-point exponent of eval_sums");
  m.def("eval_limits", &eval_limits, "structural constants of the validation kernels");
}
