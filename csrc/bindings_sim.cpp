// pybind11 bindings of the top-k cosine retrieval ops (registered from bindings.cpp via
// register_sim_ops): HIP tensors launch the gfx950 kernels on the current stream, CPU tensors run
// the host twins. Shapes, dtypes, k and the queries' lengths (they bound the LDS tables) are
// validated here, before any launch.
#define FDX_PREFIX "fdx.sim: "
#include "bindings_util.h"

#include <algorithm>

#include "sim.h"

namespace {

void chk_val(const Tensor& val, const at::Device& dev) {
  FDX_CHECK(val.device() == dev && val.is_contiguous() &&
                (val.scalar_type() == at::kFloat || val.scalar_type() == at::kDouble),
            "val must be contiguous float32 / float64 on the CSR's device");
}

// bytes of per-chunk candidates held at once; longer query batches run in several passes
constexpr int64_t kCandBudget = int64_t(256) << 20;

template <class V>
void run_norms(const Tensor& indptr, const Tensor& val, const Tensor& norms, int64_t threads) {
  const auto dev = indptr.device();
  fdx::SimNormArgs<V> a{indptr.data_ptr<int64_t>(), val.data_ptr<V>(), indptr.numel() - 1, norms.data_ptr<double>()};
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    fdx::launch_sim_norms<V>(a, stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    fdx::sim_norms_cpu<V>(a, (int)threads);
  }
}

void sim_norms(const Tensor& indptr, const Tensor& val, const Tensor& norms, int64_t threads) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk_val(val, dev);
  chk(norms, dev, at::kDouble, "norms");
  FDX_CHECK(indptr.numel() >= 1 && norms.numel() == indptr.numel() - 1, "norms needs one entry per row");
  if (val.scalar_type() == at::kFloat) run_norms<float>(indptr, val, norms, threads);
  else run_norms<double>(indptr, val, norms, threads);
}

void sim_topk(const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& norms, const Tensor& q_indptr,
              const Tensor& q_idx, const Tensor& q_val, int64_t k, const Tensor& rows_out, const Tensor& sims_out,
              int64_t chunk_rows, int64_t queries_per_pass, int64_t threads) {
  const auto dev = indptr.device();
  chk(indptr, dev, at::kLong, "indptr");
  chk(idx, dev, at::kInt, "idx");
  chk_val(val, dev);
  chk(norms, dev, at::kDouble, "norms");
  chk(q_indptr, dev, at::kLong, "q_indptr");
  chk(q_idx, dev, at::kInt, "q_idx");
  chk(q_val, dev, at::kDouble, "q_val");
  chk(rows_out, dev, at::kLong, "rows_out");
  chk(sims_out, dev, at::kDouble, "sims_out");
  if (k < 1 || k > fdx::kSimKMax) throw pybind11::value_error("fdx.sim: k must lie in 1 .. k_max");
  FDX_CHECK(indptr.numel() >= 1 && q_indptr.numel() >= 1, "indptr, q_indptr hold rows + 1 entries");
  const int64_t rows = indptr.numel() - 1, queries = q_indptr.numel() - 1;
  FDX_CHECK(idx.numel() == val.numel() && q_idx.numel() == q_val.numel(), "idx / val size");
  FDX_CHECK(norms.numel() == rows, "norms needs one entry per row");
  if (chunk_rows == 0) chunk_rows = fdx::kSimChunkRows;
  if (queries_per_pass == 0) queries_per_pass = fdx::kSimQueriesPerPass;
  FDX_CHECK(chunk_rows >= 1 && chunk_rows <= fdx::kSimMaxChunkRows, "chunk_rows out of range");
  FDX_CHECK(queries_per_pass >= 1 && queries_per_pass <= fdx::kSimQueriesPerPass, "queries_per_pass out of range");
  const int64_t k_out = std::min<int64_t>(k, rows);
  FDX_CHECK(rows_out.numel() == queries * k_out && sims_out.numel() == queries * k_out,
            "rows_out, sims_out [queries, min(k, rows)]");
  if (rows == 0 || queries == 0) return;
  int64_t longest = 0;
  {  // the queries' extents bound what the kernels read and size the LDS tables
    const Tensor qp = q_indptr.cpu();
    const int64_t* p = qp.data_ptr<int64_t>();
    FDX_CHECK(p[0] >= 0 && p[queries] <= q_idx.numel(), "q_indptr outside q_idx");
    for (int64_t q = 0; q < queries; ++q) {
      FDX_CHECK(p[q + 1] >= p[q] && p[q + 1] - p[q] <= fdx::kSimQueryCap, "a query holds 0 .. query_cap terms");
      longest = std::max(longest, p[q + 1] - p[q]);
    }
  }
  const Tensor q_norms = at::empty({queries}, norms.options());
  run_norms<double>(q_indptr, q_val, q_norms, threads);
  const int64_t chunks = fdx::sim_chunks(rows, chunk_rows);
  const int64_t cands = chunks * k;
  int64_t batch = std::max<int64_t>(1, kCandBudget / (cands * 16));
  batch = std::min(batch, std::max<int64_t>(1, (int64_t(1) << 30) / chunks));   // grid = chunks * tiles
  batch = std::max(queries_per_pass, batch / queries_per_pass * queries_per_pass);
  batch = std::min(batch, queries);
  FDX_CHECK(chunks * ((batch + queries_per_pass - 1) / queries_per_pass) < (int64_t(1) << 31), "corpus too large");
  const Tensor cand_sims = at::empty({batch * cands}, sims_out.options());
  const Tensor cand_rows = at::empty({batch * cands}, rows_out.options());
  auto run = [&](auto tag) {
    using V = decltype(tag);
    for (int64_t b0 = 0; b0 < queries; b0 += batch) {
      fdx::SimTopkArgs<V> a{};
      a.indptr = indptr.data_ptr<int64_t>();
      a.idx = idx.data_ptr<int32_t>();
      a.val = val.data_ptr<V>();
      a.norms = norms.data_ptr<double>();
      a.rows = rows;
      a.q_indptr = q_indptr.data_ptr<int64_t>() + b0;
      a.q_idx = q_idx.data_ptr<int32_t>();
      a.q_val = q_val.data_ptr<double>();
      a.q_norms = q_norms.data_ptr<double>() + b0;
      a.queries = std::min(batch, queries - b0);
      a.k = (int)k;
      a.chunk_rows = (int)chunk_rows;
      a.queries_per_pass = (int)queries_per_pass;
      a.table_cap = fdx::sim_table_cap(longest);
      a.chunks = chunks;
      a.cand_sims = cand_sims.data_ptr<double>();
      a.cand_rows = cand_rows.data_ptr<int64_t>();
      fdx::SimMergeArgs m{a.cand_sims, a.cand_rows, a.queries, cands, (int)k, (int)k_out,
                          sims_out.data_ptr<double>() + b0 * k_out, rows_out.data_ptr<int64_t>() + b0 * k_out};
      if (dev.is_cuda()) {
        c10::hip::HIPGuard guard(dev.index());
        fdx::launch_sim_topk<V>(a, stream(dev));
        C10_HIP_KERNEL_LAUNCH_CHECK();
        fdx::launch_sim_merge(m, stream(dev));
        C10_HIP_KERNEL_LAUNCH_CHECK();
      } else {
        fdx::sim_topk_cpu<V>(a, (int)threads);
        fdx::sim_merge_cpu(m, (int)threads);
      }
    }
  };
  if (val.scalar_type() == at::kFloat) run(float{}); else run(double{});
}

pybind11::dict sim_limits() {
  pybind11::dict d;
  d["k_max"] = fdx::kSimKMax;
  d["query_cap"] = fdx::kSimQueryCap;
  d["chunk_rows"] = fdx::kSimChunkRows;
  d["queries_per_pass"] = fdx::kSimQueriesPerPass;
  d["wave"] = fdx::kSimWave;
  d["block"] = fdx::kSimBlock;
  return d;
}

}  // namespace

void register_sim_ops(pybind11::module& m) {
  namespace py = pybind11;
  m.def("sim_norms", &sim_norms, "row norms of a CSR in spmv's summation order", py::arg("indptr"), py::arg("val"),
        py::arg("norms"), py::arg("threads") = 0);
  m.def("sim_topk", &sim_topk, "exact top-k cosine neighbours of a batch of CSR queries in a CSR corpus",
        py::arg("indptr"), py::arg("idx"), py::arg("val"), py::arg("norms"), py::arg("q_indptr"), py::arg("q_idx"),
        py::arg("q_val"), py::arg("k"), py::arg("rows_out"), py::arg("sims_out"), py::arg("chunk_rows") = 0,
        py::arg("queries_per_pass") = 0, py::arg("threads") = 0);
  m.def("sim_limits", &sim_limits, "structural constants of the retrieval kernels");
}
