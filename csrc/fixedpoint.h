// The exact fixed-point row pass shared by Naive Bayes (nb.h), multinomial logistic regression
// (mlr.h) and linear SVC (svc.h): its constants, the shared parts of their descriptors and the pieces
// of the pass that do not depend on the model.
//
// Device: a workgroup of four waves owns a contiguous chunk of rows, a wave one row at a time; a
// row's entries are read lane-strided and coalesced and summed with the xor butterfly. Every term is
// quantised once (nb_quant) and added as an integer: a feature of the hot set (slot_of[f] <
// hot_slots, a 2-byte table that stays in L2) adds into the workgroup's int64 LDS table with a
// 64-bit LDS atomic, every other entry goes straight to a 64-bit global atomic. The table's non-zero
// slots are flushed with global atomics when the chunk is done, so a token that occurs in every row
// costs one global atomic per workgroup instead of one per row. A few scalar sums are kept per wave
// in registers, then in LDS, and leave the workgroup as one global atomic each. The table is
// class-major [C][H] (Naive Bayes: a row adds to one class) or feature-major [H][C] (the C terms of
// an entry are adjacent; SVC is C = 1). Bad input raises a flag word.
// Host: every thread owns a range of rows and a private block, and the blocks are merged.
// Integer adds commute, so the hot set, the chunk size, the grid, the host threads and the world
// size change the speed only. The row loops themselves live with each model: they differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "common.h"

namespace fdx {

// the kNb* names are those of the first model built on the pass
constexpr int kNbWave = 64;
constexpr int kNbBlock = 256;                      // lanes of a workgroup
constexpr int kNbWaves = kNbBlock / kNbWave;
constexpr int kNbMaxClasses = kMaxClasses;
constexpr int kNbChunkRows = 1024;                 // default rows of a workgroup
constexpr int64_t kNbMaxChunkRows = 1 << 20;
constexpr int kNbTableBytes = 32 * 1024;           // default LDS table of the hot features, int64 (swept)
constexpr int kNbMaxTableBytes = 63 * 1024;        // with the scalar sums a workgroup stays within 64 KiB
constexpr int kNbKMax = 40;                        // largest scale exponent
constexpr int kNbSumBits = 61;                     // |sum| < 2^61
constexpr int kNbPrefixRows = 65536;               // rows whose document frequencies choose the hot set
constexpr uint16_t kNbCold = 0xFFFF;               // slot_of value of a feature outside the hot set

// losses (mlr_eval, svc_eval): the cap of a row's loss and the two 32-bit halves of the flag word,
// each written with ordinary stores of the value 1
constexpr double kMlrLossCap = 2048.0;             // a row's loss counts at most this much
constexpr int kMlrLossBits = 11;                   // kMlrLossCap = 2^kMlrLossBits
constexpr int64_t kMlrFlagClamped = 1;             // low half: a row's loss was not below the cap
constexpr int64_t kMlrFlagBadInput = int64_t(1) << 32;  // high half: bad input

// slots per class of an LDS table of `bytes`
constexpr int nb_hot_slots(int num_classes, int bytes = kNbTableBytes) { return bytes / (8 * num_classes); }

inline int64_t nb_chunks(int64_t rows, int64_t chunk_rows) { return (rows + chunk_rows - 1) / chunk_rows; }

// host side of the 64-lane sum (lane 0 of the xor butterfly)
inline double nb_butterfly_host(double* p) {
  for (int o = kNbWave / 2; o > 0; o >>= 1)
    for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
  return p[0];
}

// ---------------------------------------------------------------- shared descriptor parts
template <class V>
struct CsrRows {             // a CSR with a label and a weight per row
  const int64_t* indptr;     // [rows + 1]
  const int32_t* idx;
  const V* val;
  const double* labels;      // [rows]
  const double* weights;     // [rows] or nullptr (1.0)
  int64_t rows;
  int32_t F;
};

struct HotSet {              // device only (no hot set: hot_slots = 0)
  const uint16_t* slot_of;   // [F] slot of a hot feature, >= hot_slots otherwise
  const int32_t* hot_feat;   // [hot_slots] feature of a slot
  int hot_slots;             // classes * hot_slots * 8 <= kNbMaxTableBytes
  int chunk_rows;            // rows of a workgroup
};

// ---------------------------------------------------------------- launch
struct FxLaunch {
  unsigned grid;             // one workgroup per chunk of rows
  size_t lds;                // bytes of the hot table
};

// classes = 1 for a model without classes (SVC); KMeans raises the class cap and lowers the table's
inline FxLaunch fx_launch(const char* op, int classes, int min_classes, const HotSet& h, int64_t rows,
                          int max_classes = kNbMaxClasses, int max_table_bytes = kNbMaxTableBytes) {
  if (classes < min_classes || classes > max_classes || h.chunk_rows < 1 || h.hot_slots < 0 ||
      (int64_t)classes * h.hot_slots * 8 > max_table_bytes)
    throw std::runtime_error(std::string("fdx ") + op + ": classes, chunk or hot set out of range");
  return {(unsigned)nb_chunks(rows, h.chunk_rows), (size_t)classes * h.hot_slots * sizeof(uint64_t)};
}

}  // namespace fdx

#ifdef __HIPCC__
// ---------------------------------------------------------------- device pieces
namespace fdx {

using fx_u64 = unsigned long long;

__device__ __forceinline__ double fx_wave_sum(double v) {
#pragma unroll
  for (int o = kNbWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kNbWave);
  return v;
}

// rows [r0, r1) of this workgroup
__device__ __forceinline__ void fx_chunk(const HotSet& h, int64_t rows, int64_t& r0, int64_t& r1) {
  r0 = (int64_t)blockIdx.x * h.chunk_rows;
  r1 = r0 + h.chunk_rows < rows ? r0 + h.chunk_rows : rows;
}

__device__ __forceinline__ void fx_table_zero(fx_u64* table, int slots) {
  for (int i = threadIdx.x; i < slots; i += kNbBlock) table[i] = 0;
}

// slot of feature f: < hot_slots iff f is hot
__device__ __forceinline__ int fx_slot(const HotSet& h, int32_t f) {
  return h.hot_slots ? (int)h.slot_of[f] : (int)kNbCold;
}

// where class 0 of feature f adds, feature-major: table [H][C] or G [F][C] (the class-major pass
// adds one term per entry and branches on fx_slot itself: an LDS and a global atomic, no flat one)
template <int C>
__device__ __forceinline__ fx_u64* fx_dst(const HotSet& h, fx_u64* table, fx_u64* G, int32_t f) {
  const int slot = fx_slot(h, f);
  return slot < h.hot_slots ? table + slot * C : G + (int64_t)f * C;
}

// flush of the non-zero slots of a feature-major table [H][C] into G [F][C] (after a barrier)
template <int C>
__device__ __forceinline__ void fx_flush(const HotSet& h, const fx_u64* table, fx_u64* G, int32_t F) {
  for (int i = threadIdx.x; i < C * h.hot_slots; i += kNbBlock) {
    const fx_u64 v = table[i];
    if (v == 0) continue;
    const int slot = i / C;
    const int32_t f = h.hot_feat[slot];
    if ((uint32_t)f < (uint32_t)F) atomicAdd(G + (int64_t)f * C + (i - slot * C), v);
  }
}

// flush of the non-zero slots of a class-major table [C][H] into S [C][F] (after a barrier)
__device__ __forceinline__ void fx_flush_rows(const HotSet& h, const fx_u64* table, fx_u64* S, int32_t F, int C) {
  const int H = h.hot_slots;
  for (int i = threadIdx.x; i < C * H; i += kNbBlock) {
    const fx_u64 v = table[i];
    if (v == 0) continue;
    const int c = i / H;
    const int32_t f = h.hot_feat[i - c * H];
    if ((uint32_t)f < (uint32_t)F) atomicAdd(S + (int64_t)c * F + f, v);
  }
}

// a wave's scalar sum into the workgroup's (lane 0 calls; zero sums are skipped)
__device__ __forceinline__ void fx_sum_to_lds(fx_u64* sum_s, fx_u64 v) {
  if (v) atomicAdd(sum_s, v);
}

// the workgroup's scalar sum into the output (one thread per sum calls, after a barrier)
__device__ __forceinline__ void fx_sum_to_global(int64_t* dst, fx_u64 v) {
  if (v) atomicAdd(reinterpret_cast<fx_u64*>(dst), v);
}

// the two halves of the flag word; every writer stores the same value
__device__ __forceinline__ void fx_flag(int64_t* flag, bool clamped, bool bad) {
  if (clamped) reinterpret_cast<int32_t*>(flag)[0] = 1;
  if (bad) reinterpret_cast<int32_t*>(flag)[1] = 1;
}

}  // namespace fdx

#else
// ---------------------------------------------------------------- host twin pieces
#include <algorithm>
#include <atomic>
#include <vector>

#include "parallel_for.h"

namespace fdx {

// Runs flags |= body(lo, hi, wide, tail) over ranges of the rows, thread 0 on `wide` [width] and
// `tail` [ntail] themselves, every other thread on a private zeroed block [width | ntail]; then adds
// the private blocks in (the wide part in parallel) and returns the flags. At least 256 rows a thread.
template <class Body>
int64_t fx_host_pass(int64_t rows, int threads, uint64_t* wide, int64_t width, uint64_t* tail, int ntail,
                     Body&& body) {
  int T = threads <= 0 ? HostPool::get().size() : threads;
  T = (int)std::max<int64_t>(1, std::min<int64_t>(T, rows / 256));
  std::vector<std::vector<uint64_t>> priv(T > 1 ? T - 1 : 0);
  std::atomic<int64_t> flags{0};
  const int64_t per = (rows + T - 1) / T;
  parallel_for(T, T, 1, [&](int64_t lo, int64_t hi) {
    for (int64_t t = lo; t < hi; ++t) {
      uint64_t *w = wide, *s = tail;
      if (t != 0) {
        priv[t - 1].assign((size_t)(width + ntail), 0);
        w = priv[t - 1].data();
        s = w + width;
      }
      const int64_t f = body(std::min(rows, t * per), std::min(rows, (t + 1) * per), w, s);
      if (f) flags.fetch_or(f, std::memory_order_relaxed);
    }
  });
  if (T > 1)
    parallel_for(width, threads, 1 << 14, [&](int64_t lo, int64_t hi) {
      for (const auto& p : priv)
        for (int64_t i = lo; i < hi; ++i) wide[i] += p[i];
    });
  for (const auto& p : priv)
    for (int i = 0; i < ntail; ++i) tail[i] += p[width + i];
  return flags.load();
}

}  // namespace fdx
#endif
