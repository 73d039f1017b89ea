// On-device calibration scoring (the reference's utils/metrics.py:6-15, 35-80:
// neg_log_likelihood, expected_calibration_error, accuracy) of a probability
// matrix that is already resident on the device, e.g. cnf_predict's output.
// cnf_metrics ADDS the integer record documented in include/cnf.h into a
// caller-owned int64 array; the host turns the 4 + 3 * bins words into NLL,
// ECE, accuracy and the reliability diagram (cnf_hip/metrics.py).
//
// Semantics ("Scoring"): per row the prediction is the FIRST index
// of the row maximum (np.argmax) and the confidence is that maximum; bin i
// holds the row iff i * width < conf <= (i + 1) * width with the fp32
// confidence widened to double and width = 1.0 / bins formed in double.  The
// kernel compares fp32 against thr[i], the largest fp32 <= the double edge
// (computed on the host), which decides every fp32 value as the double
// comparison does.  Every sum is an integer (counts; confidences and NLL
// terms as rint(value * 2^32)), so the record is bitwise repeatable and
// independent of grid size, batch split and shard split.
//
// Mechanism: LPR lanes share a row (4 / 16 / 64 by D, coalesced column
// strides), carry (value, index) through a butterfly that prefers the smaller
// index on equal values, and lane 0 of the group adds the row into a
// per-block LDS record with integer LDS atomics; the block then adds its
// non-zero words into `record` with one integer atomic each.  The grid is at
// most kMaxBlocks blocks, so a call issues at most kMaxBlocks * (4 + 3 * bins)
// global atomics whatever B is.  No float atomics, no spin-wait, no workspace.
//
// TWIN: cnf_score.h restates Edges, the threshold loop of cnf_metrics, lds_add
// and k_metrics' per-row and flush code for the score kernels, which must
// leave the same words (tests/test_gpu_score.py).  A change to the bin rule,
// the validity rules or the fixed point here belongs there too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cnf_internal.h"

namespace cnf {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 512;
constexpr int64_t kMaxRows = 1LL << 26;  // a term is < 2^5: 2^26 rows fit the 2^-32 fixed point
constexpr int kRecMax = 4 + 3 * CNF_MAX_BINS;

struct Edges {
  float thr[CNF_MAX_BINS + 1];  // thr[i]: largest fp32 <= (double)i * (1.0 / bins)
};

__device__ __forceinline__ void lds_add(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

template <int LPR>
__global__ __launch_bounds__(kThreads) void k_metrics(const float* __restrict__ probs,
                                                      const int64_t* __restrict__ y, int D,
                                                      int bins, int64_t B, Edges e,
                                                      int64_t* __restrict__ record) {
  constexpr int RPB = kThreads / LPR;  // rows per block and pass
  __shared__ long long rec[kRecMax];
  const int nwords = 4 + 3 * bins;
  for (int i = threadIdx.x; i < nwords; i += kThreads) rec[i] = 0;
  __syncthreads();

  const int sub = threadIdx.x % LPR;  // lane within the row's group
  const int grp = threadIdx.x / LPR;
  long long nll_fx = 0;
  int n_rows = 0, n_invalid = 0, n_correct = 0;

  // the loop bound is uniform over the block: every lane takes part in the shuffles
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < B; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + grp;
    const bool live = r < B;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    unsigned pyb = 0;  // bits of p[y]: non-zero in at most one lane of the group
    int bad = 0;
    int64_t label = -1;
    if (live) {
      label = y[r];
      const float* row = probs + r * D;
      for (int c = sub; c < D; c += LPR) {
        const float v = __builtin_nontemporal_load(row + c);
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
      // -log(p[y] + 1e-7) on the widened value (metrics.py:15), in double: the
      // term carries no fp32 rounding of its own
      const double arg = (double)__uint_as_float(pyb) + 1e-7;
      const bool valid = label >= 0 && label < (int64_t)D && !bad && arg > 0.0;
      if (!valid) {
        ++n_invalid;
      } else {
        ++n_rows;
        nll_fx += __double2ll_rn(-log(arg) * 4294967296.0);
        const int hit = (int64_t)bidx == label;
        n_correct += hit;
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

  // the four scalar words: one butterfly per wave, one LDS add per wave and word
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nll_fx += __shfl_xor(nll_fx, o, 64);
    n_rows += __shfl_xor(n_rows, o, 64);
    n_invalid += __shfl_xor(n_invalid, o, 64);
    n_correct += __shfl_xor(n_correct, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    lds_add(&rec[0], n_rows);
    lds_add(&rec[1], n_invalid);
    lds_add(&rec[2], nll_fx);
    lds_add(&rec[3], n_correct);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nwords; i += kThreads) {
    const long long v = rec[i];
    if (v != 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(record + i), (unsigned long long)v);
  }
}

int check_shape(int32_t dim, int32_t bins) {
  if (dim < 2 || bins < 1 || bins > CNF_MAX_BINS) return CNF_ERR_DESC;
  if (dim > CNF_MAX_DIM) return CNF_ERR_UNSUPPORTED;
  return CNF_OK;
}

}  // namespace
}  // namespace cnf

extern "C" int cnf_metrics_record_words(int32_t bins, int64_t* words) {
  if (!words) return CNF_ERR_NULL;
  if (bins < 1 || bins > CNF_MAX_BINS) return CNF_ERR_DESC;
  *words = 4 + 3 * (int64_t)bins;
  return CNF_OK;
}

extern "C" int cnf_metrics_workspace_bytes(int32_t dim, int32_t bins, int64_t B, size_t* bytes) {
  using namespace cnf;
  if (!bytes) return CNF_ERR_NULL;
  const int st = check_shape(dim, bins);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  *bytes = 0;  // blocks add into the record with integer atomics: no partials
  return CNF_OK;
}

extern "C" int cnf_metrics(const float* probs, const int64_t* y, int32_t dim, int32_t bins,
                           int64_t B, int64_t* record, void* workspace, size_t workspace_bytes,
                           void* stream) {
  using namespace cnf;
  CNF_RANGE("cnf_metrics");
  (void)workspace;
  (void)workspace_bytes;
  const int st = check_shape(dim, bins);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!record || (B > 0 && (!probs || !y))) return CNF_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(probs) & 3) || (reinterpret_cast<uintptr_t>(y) & 7) ||
      (reinterpret_cast<uintptr_t>(record) & 7))
    return CNF_ERR_ALIGN;
  if (B == 0) return CNF_OK;
  Edges e;
  const double width = 1.0 / bins;  // metrics.py:57
  for (int i = 0; i <= CNF_MAX_BINS; ++i) {
    if (i > bins) {
      e.thr[i] = INFINITY;
      continue;
    }
    const double edge = i * width;  // metrics.py:61
    float t = (float)edge;
    if ((double)t > edge) t = std::nextafterf(t, -INFINITY);
    e.thr[i] = t;
  }
  const int lpr = dim <= 16 ? 4 : dim <= 64 ? 16 : 64;
  const int64_t rpb = kThreads / lpr;
  const unsigned blocks = (unsigned)std::min<int64_t>(kMaxBlocks, (B + rpb - 1) / rpb);
  const hipStream_t s = (hipStream_t)stream;
  if (lpr == 4)
    hipLaunchKernelGGL(k_metrics<4>, dim3(blocks), dim3(kThreads), 0, s, probs, y, dim, bins, B, e,
                       record);
  else if (lpr == 16)
    hipLaunchKernelGGL(k_metrics<16>, dim3(blocks), dim3(kThreads), 0, s, probs, y, dim, bins, B,
                       e, record);
  else
    hipLaunchKernelGGL(k_metrics<64>, dim3(blocks), dim3(kThreads), 0, s, probs, y, dim, bins, B,
                       e, record);
  return launch_status();
}
