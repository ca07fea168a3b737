// Argument checks and dispatch shared by the bindings_*.cpp files. The error prefix is the header's
// parameter: a binding file defines FDX_PREFIX (for instance "fdx.nb: ") before it includes this
// header, and every check below raises with that prefix. Everything here has internal linkage, so
// each binding file gets its own copy with its own prefix.
#pragma once
#ifndef FDX_PREFIX
#error "define FDX_PREFIX (the error prefix of this binding file) before including bindings_util.h"
#endif

#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "fixedpoint.h"

#define FDX_CHECK(cond, msg) TORCH_CHECK(cond, FDX_PREFIX, msg)

namespace {

using at::Tensor;

inline void chk(const Tensor& t, const at::Device& dev, at::ScalarType st, const char* name) {
  FDX_CHECK(t.device() == dev, std::string(name) + " on wrong device");
  FDX_CHECK(t.is_contiguous(), std::string(name) + " must be contiguous");
  FDX_CHECK(t.scalar_type() == st, std::string(name) + " has wrong dtype");
}

inline hipStream_t stream(const at::Device& d) { return c10::hip::getCurrentHIPStream(d.index()).stream(); }

// an optional per-row output of doubles: its pointer, or nullptr
inline double* rows_out(const c10::optional<Tensor>& t, const at::Device& dev, int64_t numel, const char* name) {
  if (!t) return nullptr;
  chk(*t, dev, at::kDouble, name);
  FDX_CHECK(t->numel() == numel, std::string(name) + " has the wrong size");
  return t->data_ptr<double>();
}

// Dtypes and sizes of a CSR; returns its rows. With `extents` the row pointers' extremes are read
// back too (they bound what the kernels read): a fit pass pays that small copy once, a scorer
// trusts its column as spmv does. Row pointers outside idx raise through FDX_CHECK, or a ValueError
// that names `value_error_op` where one is given.
inline int64_t chk_csr(const Tensor& indptr, const Tensor& idx, const Tensor& val, bool extents,
                       const char* value_error_op = nullptr) {
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
    const bool ok = e[0] >= 0 && e[1] <= idx.numel();
    if (!ok && value_error_op)
      throw pybind11::value_error(std::string(FDX_PREFIX) + value_error_op + ": indptr must stay within idx");
    FDX_CHECK(ok, "indptr must stay within idx");
  }
  return indptr.numel() - 1;
}

inline void chk_row_labels(const Tensor& labels, const c10::optional<Tensor>& weights, const at::Device& dev,
                           int64_t rows) {
  chk(labels, dev, at::kDouble, "labels");
  FDX_CHECK(labels.numel() == rows, "labels needs one entry per row");
  if (weights) {
    chk(*weights, dev, at::kDouble, "weights");
    FDX_CHECK(weights->numel() == rows, "weights needs one entry per row");
  }
}

inline void chk_classes(int64_t C) {
  if (C < 2 || C > fdx::kNbMaxClasses)
    throw pybind11::value_error(std::string(FDX_PREFIX) + "the class count must lie in 2 .. max_classes");
}

inline void chk_scale_exponents(int64_t k, int64_t k2) {
  FDX_CHECK(k >= 0 && k <= fdx::kNbKMax && k2 >= 0 && k2 <= fdx::kNbKMax, "scale exponents lie in 0 .. k_max");
}

// 0 = the default; the chunks of `rows` must fit a grid
inline int64_t chunk_rows_or_default(int64_t chunk_rows, int64_t rows) {
  if (chunk_rows == 0) chunk_rows = fdx::kNbChunkRows;
  FDX_CHECK(chunk_rows >= 1 && chunk_rows <= fdx::kNbMaxChunkRows, "chunk_rows out of range");
  FDX_CHECK(fdx::nb_chunks(rows, chunk_rows) < (int64_t(1) << 31), "too many row chunks");
  return chunk_rows;
}

// the hot set of F features and C classes (C = 1: none); returns hot_slots, 0 without a hot set
inline int64_t chk_hot_set(const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat,
                           const at::Device& dev, int64_t F, int64_t C) {
  if (!slot_of && !hot_feat) return 0;
  FDX_CHECK(slot_of && hot_feat, "slot_of and hot_feat come together");
  chk(*slot_of, dev, at::kShort, "slot_of");
  chk(*hot_feat, dev, at::kInt, "hot_feat");
  FDX_CHECK(slot_of->numel() == F, "slot_of needs one entry per feature");
  const int64_t hot_slots = hot_feat->numel();
  FDX_CHECK(C * hot_slots * 8 <= fdx::kNbMaxTableBytes, "the hot set exceeds the LDS table");
  return hot_slots;
}

// the shared descriptor parts of fixedpoint.h from checked arguments
template <class V>
void fill_csr_rows(fdx::CsrRows<V>& a, const Tensor& indptr, const Tensor& idx, const Tensor& val, const Tensor& labels,
                   const c10::optional<Tensor>& weights, int64_t F) {
  a.indptr = indptr.data_ptr<int64_t>();
  a.idx = idx.data_ptr<int32_t>();
  a.val = val.data_ptr<V>();
  a.labels = labels.data_ptr<double>();
  a.weights = weights ? weights->data_ptr<double>() : nullptr;
  a.rows = indptr.numel() - 1;
  a.F = (int32_t)F;
}

inline void fill_hot_set(fdx::HotSet& h, const c10::optional<Tensor>& slot_of, const c10::optional<Tensor>& hot_feat,
                         int64_t hot_slots, int64_t chunk_rows) {
  h.slot_of = hot_slots ? reinterpret_cast<const uint16_t*>(slot_of->data_ptr<int16_t>()) : nullptr;
  h.hot_feat = hot_slots ? hot_feat->data_ptr<int32_t>() : nullptr;
  h.hot_slots = (int)hot_slots;
  h.chunk_rows = (int)chunk_rows;
}

// fn(float{}) or fn(double{}) by the dtype of val
template <class Fn>
void dispatch_val(const Tensor& val, Fn&& fn) {
  if (val.scalar_type() == at::kFloat) fn(float{}); else fn(double{});
}

// launch(stream) on a HIP device (guarded, on the current stream, launch checked), cpu() on the host
template <class Launch, class Cpu>
void run_on(const at::Device& dev, Launch&& launch, Cpu&& cpu) {
  if (dev.is_cuda()) {
    c10::hip::HIPGuard guard(dev.index());
    launch(stream(dev));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    cpu();
  }
}

// the *_limits() entries of the fixed-point row pass; `loss` adds those of the capped losses
inline pybind11::dict pass_limits(bool loss) {
  pybind11::dict d;
  d["chunk_rows"] = fdx::kNbChunkRows;
  d["table_bytes"] = fdx::kNbTableBytes;
  d["max_table_bytes"] = fdx::kNbMaxTableBytes;
  d["k_max"] = fdx::kNbKMax;
  d["sum_bits"] = fdx::kNbSumBits;
  d["wave"] = fdx::kNbWave;
  d["block"] = fdx::kNbBlock;
  if (loss) {
    d["loss_cap"] = fdx::kMlrLossCap;
    d["loss_bits"] = fdx::kMlrLossBits;
    d["flag_clamped"] = fdx::kMlrFlagClamped;
    d["flag_bad_input"] = fdx::kMlrFlagBadInput;
  }
  return d;
}

}  // namespace
