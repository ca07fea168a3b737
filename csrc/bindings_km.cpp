// pybind11 bindings of the KMeans ops (registered from bindings.cpp via register_km_ops): HIP tensors
// launch the gfx950 kernels on the current stream, CPU tensors run the host twins. Shapes, dtypes,
// the center count, the measure, the scale exponents and the hot set's size (it sizes the LDS table)
// are validated here (bindings_util.h), before any launch.
#define FDX_PREFIX "fdx.km: "
#include "bindings_util.h"
#include "km.h"

namespace {

void chk_centers(int64_t K, int64_t measure) {
  if (K < 2 || K > fdx::kKmMaxK)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the center count must lie in 2 .. max_k");
  if (measure != fdx::kKmEuclidean && measure != fdx::kKmCosine)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the measure is 0 (euclidean) or 1 (cosine)");
}

// out holds [S (K F) |] Wq (K) | cnt (K) | costq | flag
void km_step(const Tensor& indptr, const Tensor& idx, const Tensor& val, const c10::optional<Tensor>& weights,
             const Tensor& CT, const Tensor& cn, int64_t K, int64_t measure, int64_t k, int64_t kw, int64_t kc,
             const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat, const Tensor& out, bool sums,
             const c10::optional<Tensor>& assign, const c10::optional<Tensor>& dist, int64_t chunk_rows,
             int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, true);
  chk_centers(K, measure);
  const int64_t Kp = fdx::km_padded((int)K);
  chk(CT, dev, at::kDouble, "CT");
  chk(cn, dev, at::kDouble, "cn");
  FDX_CHECK(CT.dim() == 2 && CT.size(1) == Kp && CT.size(0) >= 1 && CT.size(0) < (int64_t(1) << 31),
            "CT is [F, Kp], Kp = K rounded up to the tile");
  FDX_CHECK(cn.numel() == Kp, "cn is [Kp]");
  const int64_t F = CT.size(0);
  if (weights) {
    chk(*weights, dev, at::kDouble, "weights");
    FDX_CHECK(weights->numel() == rows, "weights needs one entry per row");
  }
  chk_scale_exponents(k, kw);
  chk_scale_exponents(kc, kc);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == (sums ? K * F : 0) + 2 * K + 2, "out holds [K F +] 2 K + 2 sums");
  if (assign) {
    chk(*assign, dev, at::kInt, "assign");
    FDX_CHECK(assign->numel() == rows, "assign needs one entry per row");
  }
  double* const dist_p = rows_out(dist, dev, rows, "dist");
  chunk_rows = chunk_rows_or_default(chunk_rows, rows);
  int64_t hot_slots = 0;
  if (sums) {
    hot_slots = chk_hot_set(slot_of, hot_feat, dev, F, K);
    FDX_CHECK(K * hot_slots * 8 <= fdx::kKmMaxTableBytes, "the hot set exceeds the LDS table");
  }
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::KmStepArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.labels = nullptr;
    a.weights = weights ? weights->data_ptr<double>() : nullptr;
    a.rows = rows;
    a.F = (int32_t)F;
    fill_hot_set(a, slot_of, hot_feat, hot_slots, chunk_rows);
    a.K = (int)K;
    a.Kp = (int)Kp;
    a.measure = (int)measure;
    a.k = (int)k;
    a.kw = (int)kw;
    a.kc = (int)kc;
    a.CT = CT.data_ptr<double>();
    a.cn = cn.data_ptr<double>();
    int64_t* p = out.data_ptr<int64_t>();
    a.S = sums ? p : nullptr;
    a.Wq = p + (sums ? K * F : 0);
    a.cnt = a.Wq + K;
    a.costq = a.cnt + K;
    a.flag = a.costq + 1;
    a.assign = assign ? assign->data_ptr<int32_t>() : nullptr;
    a.dist = dist_p;
    run_on(dev, [&](hipStream_t s) { fdx::launch_km_step<V>(a, s); }, [&] { fdx::km_step_cpu<V>(a, (int)threads); });
  });
}

void km_centers(const Tensor& S, const Tensor& Wq, const Tensor& CT_old, int64_t K, int64_t k, int64_t kw,
                int64_t measure, const Tensor& CT_new, const Tensor& cn_new, const Tensor& moved2, int64_t threads) {
  const auto dev = S.device();
  chk_centers(K, measure);
  const int64_t Kp = fdx::km_padded((int)K);
  chk(S, dev, at::kLong, "S");
  chk(Wq, dev, at::kLong, "Wq");
  chk(CT_old, dev, at::kDouble, "CT_old");
  chk(CT_new, dev, at::kDouble, "CT_new");
  chk(cn_new, dev, at::kDouble, "cn_new");
  chk(moved2, dev, at::kDouble, "moved2");
  FDX_CHECK(CT_old.dim() == 2 && CT_old.size(1) == Kp && CT_old.size(0) >= 1 && CT_old.size(0) < (int64_t(1) << 31),
            "CT_old is [F, Kp], Kp = K rounded up to the tile");
  const int64_t F = CT_old.size(0);
  FDX_CHECK(CT_new.dim() == 2 && CT_new.size(0) == F && CT_new.size(1) == Kp, "CT_new is [F, Kp]");
  FDX_CHECK(S.numel() == K * F && Wq.numel() == K && cn_new.numel() == Kp && moved2.numel() == K,
            "S [K, F], Wq [K], cn_new [Kp], moved2 [K]");
  FDX_CHECK(CT_new.data_ptr() != CT_old.data_ptr(), "CT_new and CT_old are two buffers");
  chk_scale_exponents(k, kw);
  fdx::KmCentersArgs a{(int)K, (int)Kp, (int32_t)F, (int)measure, (int)k, (int)kw, S.data_ptr<int64_t>(),
                       Wq.data_ptr<int64_t>(), CT_old.data_ptr<double>(), CT_new.data_ptr<double>(),
                       cn_new.data_ptr<double>(), moved2.data_ptr<double>()};
  run_on(dev, [&](hipStream_t s) { fdx::launch_km_centers(a, s); }, [&] { fdx::km_centers_cpu(a, (int)threads); });
}

pybind11::dict km_limits() {
  pybind11::dict d = pass_limits(false);
  d["max_k"] = fdx::kKmMaxK;
  d["tile"] = fdx::kKmTile;
  d["max_table_bytes"] = fdx::kKmMaxTableBytes;
  d["centers_block"] = fdx::kKmCentersBlock;
  d["prefix_rows"] = fdx::kNbPrefixRows;
  return d;
}

}  // namespace

void register_km_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("km_step", &km_step,
        "one Lloyd evaluation of a CSR: assignments and the exact fixed-point sums ([S,] Wq, cnt, costq, flag in one "
        "int64 block)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("weights"), py::arg("CT"), py::arg("cn"), py::arg("K"),
        py::arg("measure"), py::arg("k"), py::arg("kw"), py::arg("kc"), py::arg("slot_of"), py::arg("hot_feat"),
        py::arg("out"), py::arg("sums"), py::arg("assign"), py::arg("dist"), py::arg("chunk_rows") = 0,
        py::arg("threads") = 0);
  m.def("km_centers", &km_centers, "the centers, their squared norms and the squared moves from the summed S and Wq",
        py::arg("S"), py::arg("Wq"), py::arg("CT_old"), py::arg("K"), py::arg("k"), py::arg("kw"), py::arg("measure"),
        py::arg("CT_new"), py::arg("cn_new"), py::arg("moved2"), py::arg("threads") = 0);
  m.def("km_limits", &km_limits, "structural constants of the KMeans kernels");
}
