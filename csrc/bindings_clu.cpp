// pybind11 bindings of the bisecting KMeans and silhouette ops (registered from bindings.cpp via
// register_clu_ops): HIP tensors launch the gfx950 kernels on the current stream, CPU tensors run the
// host twins. Shapes, dtypes, the width and the group count, the measure, the scale exponents and
// the hot set's size (it sizes the LDS table) are validated here (bindings_util.h), before any launch.
#define FDX_PREFIX "fdx.clu: "
#include "bindings_util.h"
#include "clu.h"

namespace {

void chk_measure(int64_t measure) {
  if (measure != fdx::kKmEuclidean && measure != fdx::kKmCosine)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the measure is 0 (euclidean) or 1 (cosine)");
}

void chk_weights(const c10::optional<Tensor>& weights, const at::Device& dev, int64_t rows) {
  if (!weights) return;
  chk(*weights, dev, at::kDouble, "weights");
  FDX_CHECK(weights->numel() == rows, "weights needs one entry per row");
}

// out holds [S (K F) |] Wq (K) | cnt (K) | costq (K) | flag
void km_group_step(const Tensor& indptr, const Tensor& idx, const Tensor& val, const c10::optional<Tensor>& weights,
                   const Tensor& group, int64_t W, int64_t G, const Tensor& CT, const Tensor& cn, int64_t measure,
                   int64_t k, int64_t kw, int64_t kc, const c10::optional<Tensor>& slot_of,
                   const c10::optional<Tensor>& hot_feat, const Tensor& out, bool sums,
                   const c10::optional<Tensor>& assign, const c10::optional<Tensor>& dist, int64_t chunk_rows,
                   int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, true);
  if ((W != 1 && W != 2) || G < 1 || W * G > fdx::kKmMaxK)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the width is 1 or 2 and width * groups at most max_k");
  chk_measure(measure);
  const int64_t K = fdx::clu_centers((int)W, (int)G), Kp = fdx::km_padded((int)K);
  chk(group, dev, at::kInt, "group");
  FDX_CHECK(group.numel() == rows, "group needs one entry per row");
  chk(CT, dev, at::kDouble, "CT");
  chk(cn, dev, at::kDouble, "cn");
  FDX_CHECK(CT.dim() == 2 && CT.size(1) == Kp && CT.size(0) >= 1 && CT.size(0) < (int64_t(1) << 31),
            "CT is [F, Kp], Kp = K rounded up to the tile");
  FDX_CHECK(reinterpret_cast<uintptr_t>(CT.data_ptr()) % 16 == 0, "CT is 16-byte aligned");
  FDX_CHECK(cn.numel() == Kp, "cn is [Kp]");
  const int64_t F = CT.size(0);
  chk_weights(weights, dev, rows);
  chk_scale_exponents(k, kw);
  chk_scale_exponents(kc, kc);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == (sums ? K * F : 0) + 3 * K + 1, "out holds [K F +] 3 K + 1 sums");
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
    fdx::KmGroupArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.labels = nullptr;
    a.weights = weights ? weights->data_ptr<double>() : nullptr;
    a.rows = rows;
    a.F = (int32_t)F;
    fill_hot_set(a, slot_of, hot_feat, hot_slots, chunk_rows);
    a.W = (int)W;
    a.G = (int)G;
    a.K = (int)K;
    a.Kp = (int)Kp;
    a.measure = (int)measure;
    a.k = (int)k;
    a.kw = (int)kw;
    a.kc = (int)kc;
    a.group = group.data_ptr<int32_t>();
    a.CT = CT.data_ptr<double>();
    a.cn = cn.data_ptr<double>();
    int64_t* p = out.data_ptr<int64_t>();
    a.S = sums ? p : nullptr;
    a.Wq = p + (sums ? K * F : 0);
    a.cnt = a.Wq + K;
    a.costq = a.cnt + K;
    a.flag = a.costq + K;
    a.assign = assign ? assign->data_ptr<int32_t>() : nullptr;
    a.dist = dist_p;
    run_on(dev, [&](hipStream_t s) { fdx::launch_km_group_step<V>(a, s); },
           [&] { fdx::km_group_step_cpu<V>(a, (int)threads); });
  });
}

// out holds silq | wq | flag
void sil_score(const Tensor& indptr, const Tensor& idx, const Tensor& val, const c10::optional<Tensor>& weights,
               const Tensor& label, int64_t K, const Tensor& MT, const Tensor& psi, const Tensor& nw, const Tensor& cnt,
               int64_t measure, int64_t ks, int64_t kw, const Tensor& out, const c10::optional<Tensor>& s,
               int64_t chunk_rows, int64_t threads) {
  const auto dev = indptr.device();
  const int64_t rows = chk_csr(indptr, idx, val, true);
  if (K < 2 || K > fdx::kKmMaxK)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the cluster count must lie in 2 .. max_k");
  chk_measure(measure);
  const int64_t Kp = fdx::km_padded((int)K);
  chk(label, dev, at::kInt, "label");
  FDX_CHECK(label.numel() == rows, "label needs one entry per row");
  chk(MT, dev, at::kDouble, "MT");
  chk(psi, dev, at::kDouble, "psi");
  chk(nw, dev, at::kDouble, "nw");
  chk(cnt, dev, at::kInt, "cnt");
  FDX_CHECK(MT.dim() == 2 && MT.size(1) == Kp && MT.size(0) >= 1 && MT.size(0) < (int64_t(1) << 31),
            "MT is [F, Kp], Kp = K rounded up to the tile");
  FDX_CHECK(psi.numel() == Kp && nw.numel() == Kp && cnt.numel() == Kp, "psi, nw and cnt are [Kp]");
  const int64_t F = MT.size(0);
  chk_weights(weights, dev, rows);
  chk_scale_exponents(ks, kw);
  chk(out, dev, at::kLong, "out");
  FDX_CHECK(out.numel() == 3, "out holds silq, wq and the flag");
  double* const s_p = rows_out(s, dev, rows, "s");
  chunk_rows = chunk_rows_or_default(chunk_rows, rows);
  dispatch_val(val, [&](auto tag) {
    using V = decltype(tag);
    fdx::SilArgs<V> a{};
    a.indptr = indptr.data_ptr<int64_t>();
    a.idx = idx.data_ptr<int32_t>();
    a.val = val.data_ptr<V>();
    a.labels = nullptr;
    a.weights = weights ? weights->data_ptr<double>() : nullptr;
    a.rows = rows;
    a.F = (int32_t)F;
    fill_hot_set(a, c10::nullopt, c10::nullopt, 0, chunk_rows);
    a.K = (int)K;
    a.Kp = (int)Kp;
    a.measure = (int)measure;
    a.ks = (int)ks;
    a.kw = (int)kw;
    a.label = label.data_ptr<int32_t>();
    a.MT = MT.data_ptr<double>();
    a.psi = psi.data_ptr<double>();
    a.nw = nw.data_ptr<double>();
    a.cnt = cnt.data_ptr<int32_t>();
    int64_t* p = out.data_ptr<int64_t>();
    a.silq = p;
    a.wq = p + 1;
    a.flag = p + 2;
    a.s = s_p;
    run_on(dev, [&](hipStream_t st) { fdx::launch_sil_score<V>(a, st); }, [&] { fdx::sil_score_cpu<V>(a, (int)threads); });
  });
}

pybind11::dict clu_limits() {
  pybind11::dict d = pass_limits(false);
  d["max_k"] = fdx::kKmMaxK;
  d["max_width"] = fdx::kCluMaxWidth;
  d["tile"] = fdx::kKmTile;
  d["max_table_bytes"] = fdx::kKmMaxTableBytes;
  return d;
}

}  // namespace

void register_clu_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("km_group_step", &km_group_step,
        "a Lloyd step in which group[r] names the W candidate centers of row r: assignments and the exact fixed-point "
        "sums ([S,] Wq, cnt, costq per cluster, flag in one int64 block)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("weights"), py::arg("group"), py::arg("W"),
        py::arg("G"), py::arg("CT"), py::arg("cn"), py::arg("measure"), py::arg("k"), py::arg("kw"), py::arg("kc"),
        py::arg("slot_of"), py::arg("hot_feat"), py::arg("out"), py::arg("sums"), py::arg("assign"), py::arg("dist"),
        py::arg("chunk_rows") = 0, py::arg("threads") = 0);
  m.def("sil_score", &sil_score,
        "Spark's silhouette coefficient of every row from per-cluster statistics, summed exactly (silq, wq, flag)",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("weights"), py::arg("label"), py::arg("K"),
        py::arg("MT"), py::arg("psi"), py::arg("nw"), py::arg("cnt"), py::arg("measure"), py::arg("ks"), py::arg("kw"),
        py::arg("out"), py::arg("s"), py::arg("chunk_rows") = 0, py::arg("threads") = 0);
  m.def("clu_limits", &clu_limits, "structural constants of the bisecting KMeans and silhouette kernels");
}
