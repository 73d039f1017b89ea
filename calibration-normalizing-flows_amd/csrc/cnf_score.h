// The scoring epilogue of a predict kernel's score variant (today
// cnf_planar_score; written for the row layout the planar, scaling and PAV
// predict kernels share): what k_metrics (cnf_metrics.hip) does per row,
// applied to the fp32 probabilities a predict kernel holds in registers
// immediately before its store, so the [B][D] matrix never goes to memory.
// The record layout, the validity rules and the "ADDS into record" contract
// are those include/cnf.h documents for cnf_metrics; a score kernel and
// predict + cnf_metrics give the same words.
//
// This file is the TWIN of k_metrics and of cnf_metrics' host threshold loop:
// Edges, make_edges, lds_add, kMaxRows, the body of row() after the column
// scan and flush() restate them line for line (k_metrics keeps its own copy so
// that its code stays as it is).  A change to one belongs in the other; the
// word-for-word tests of tests/test_gpu_score.py are what holds them together.
//
// Row layout: LPR lanes share a row, lane `sub` holds columns sub + k * LPR,
// k < CPL.  Columns c >= D are padding: they enter neither the maximum, p[y]
// nor the non-finite flag.
//
// A score kernel calls, with bounds that are uniform over the block (every
// lane reaches the shuffles and the barriers):
//   init(rec, bins)                       once, before the row loop
//   row<LPR, CPL>(p, sub, D, ...)         once per row pass, by every lane
//   flush(rec, bins, acc, record)         once, after the row loop
// No float atomics, no spin-wait, no workspace: integer LDS atomics per row,
// one integer global atomic per block and non-zero word.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cnf.h"

namespace cnf {
namespace score {

constexpr int kRecWords = 4 + 3 * CNF_MAX_BINS;
constexpr int64_t kMaxRows = 1LL << 26;  // as cnf_metrics: 2^26 terms fit the 2^-32 fixed point

struct Edges {
  float thr[CNF_MAX_BINS + 1];  // thr[i]: largest fp32 <= (double)i * (1.0 / bins)
};

// What a score kernel takes in place of its predict sibling's output pointers.
struct Args {
  const int64_t* y;
  int64_t* record;
  int bins;
  Edges e;
};

// The four scalar words of the record, kept per lane until flush().
struct Acc {
  long long nll_fx = 0;
  int n_rows = 0, n_invalid = 0, n_correct = 0;
};

// The thresholds as cnf_metrics builds them (utils/metrics.py:57-61).
inline Edges make_edges(int bins) {
  Edges e;
  const double width = 1.0 / bins;
  for (int i = 0; i <= CNF_MAX_BINS; ++i) {
    if (i > bins) {
      e.thr[i] = INFINITY;
      continue;
    }
    const double edge = i * width;
    float t = (float)edge;
    if ((double)t > edge) t = std::nextafterf(t, -INFINITY);
    e.thr[i] = t;
  }
  return e;
}

// The argument checks a score entry point adds to its predict sibling's; runs
// before any HIP call.
inline int check_args(int32_t dim, int32_t bins, int64_t B, const int64_t* y,
                      const int64_t* record) {
  if (dim < 2 || bins < 1 || bins > CNF_MAX_BINS) return CNF_ERR_DESC;
  if (dim > CNF_MAX_DIM) return CNF_ERR_UNSUPPORTED;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!record || (B > 0 && !y)) return CNF_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(y) & 7) || (reinterpret_cast<uintptr_t>(record) & 7))
    return CNF_ERR_ALIGN;
  return CNF_OK;
}

inline Args make_args(const int64_t* y, int32_t bins, int64_t* record) {
  Args a;
  a.y = y;
  a.record = record;
  a.bins = bins;
  a.e = make_edges(bins);
  return a;
}

__device__ __forceinline__ void lds_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// Zero the block's LDS record (kRecWords words).
__device__ __forceinline__ void init(long long* rec, int bins) {
  const int nwords = 4 + 3 * bins;
  for (int i = threadIdx.x; i < nwords; i += blockDim.x) rec[i] = 0;
  __syncthreads();
}

// One row per lane group: p[k] is the fp32 probability of column sub + k * LPR
// (anything for a column >= D), label the row's label (unused unless live).
template <int LPR, int CPL>
__device__ __forceinline__ void row(const float (&p)[CPL], int sub, int D, int64_t label,
                                    bool live, int bins, const Edges& e, long long* rec,
                                    Acc& acc) {
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  unsigned pyb = 0;  // bits of p[y]: non-zero in at most one lane of the group
  int bad = 0;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = sub + k * LPR;
    if (c < D) {
      const float v = p[k];
      bad |= !(fabsf(v) < INFINITY);  // NaN or +-inf
      if (v > best) {                 // ascending c: the first maximum stays
        best = v;
        bidx = c;
      }
      if ((int64_t)c == label) pyb = __float_as_uint(v);  // selected by comparison, never indexed
    }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bidx, o, 64);
    if (ov > best || (ov == best && oi < bidx)) {
      best = ov;
      bidx = oi;
    }
    pyb |= (unsigned)__shfl_xor((int)pyb, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if (live && sub == 0) {
    const double arg = (double)__uint_as_float(pyb) + 1e-7;
    const bool valid = label >= 0 && label < (int64_t)D && !bad && arg > 0.0;
    if (!valid) {
      ++acc.n_invalid;
    } else {
      ++acc.n_rows;
      acc.nll_fx += __double2ll_rn(-log(arg) * 4294967296.0);
      const int hit = (int64_t)bidx == label;
      acc.n_correct += hit;
      int k = 0;  // edges below the confidence
      for (int i = 0; i <= bins; ++i) k += e.thr[i] < best;
      if (k >= 1 && k <= bins) {
        const int b = k - 1;
        lds_add(&rec[4 + b], 1);
        lds_add(&rec[4 + bins + b], __double2ll_rn((double)best * 4294967296.0));
        if (hit) lds_add(&rec[4 + 2 * bins + b], 1);
      }
    }
  }
}

// The block's words into `record`: one butterfly per wave and scalar word,
// one LDS add per wave and word, then one global atomic per non-zero word.
__device__ __forceinline__ void flush(long long* rec, int bins, Acc acc,
                                      int64_t* __restrict__ record) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc.nll_fx += __shfl_xor(acc.nll_fx, o, 64);
    acc.n_rows += __shfl_xor(acc.n_rows, o, 64);
    acc.n_invalid += __shfl_xor(acc.n_invalid, o, 64);
    acc.n_correct += __shfl_xor(acc.n_correct, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    lds_add(&rec[0], acc.n_rows);
    lds_add(&rec[1], acc.n_invalid);
    lds_add(&rec[2], acc.nll_fx);
    lds_add(&rec[3], acc.n_correct);
  }
  __syncthreads();
  const int nwords = 4 + 3 * bins;
  for (int i = threadIdx.x; i < nwords; i += blockDim.x) {
    const long long v = rec[i];
    if (v != 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(record + i), (unsigned long long)v);
  }
}

}  // namespace score
}  // namespace cnf
