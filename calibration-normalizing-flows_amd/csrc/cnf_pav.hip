// Isotonic (pool-adjacent-violators) calibration, the device half: the fused
// predict of the reference's PAVCalibrator (calibrators.py:208-236, one
// IsotonicRegression(y_min=0, y_max=1, out_of_bounds='clip') per class on the
// class's softmax score) from per-class threshold tables that the host fit
// (cnf_hip/pav.py) uploads.  include/cnf.h documents the entry point;
// DESIGN.md ("Isotonic calibration") the measurements.
//
// cnf_pav_predict: one launch; per row the centred float64 softmax, per class
// the clipped look-up with SciPy interp1d's linear formula, the row
// normalisation and Calibrator.predict's prior correction, rounded once to
// fp32.  The tables are staged in LDS when D * cap entries fit kLdsEntries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cnf_internal.h"

namespace cnf {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxRows = 1LL << 26;
constexpr int kLdsEntries = 2048;  // D * cap (x, y) pairs staged in LDS (32 KiB)

// ---- row softmax, as cnf_scaling.hip: LPR lanes share a row ------------------
template <int LPR>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int LPR>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
template <int LPR, int CPL>
__device__ __forceinline__ void softmax_group(double (&t)[CPL]) {
  double m = t[0];
#pragma unroll
  for (int k = 1; k < CPL; ++k) m = fmax(m, t[k]);
  m = group_max<LPR>(m);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    t[k] = exp(t[k] - m);
    s += t[k];
  }
  s = group_sum<LPR>(s);
#pragma unroll
  for (int k = 0; k < CPL; ++k) t[k] = t[k] / s;
}

// t[k] = softmax(x - mean(x))[sub + k * LPR] of row r (-inf columns beyond D give 0)
template <int LPR, int CPL>
__device__ __forceinline__ void row_scores(const float* __restrict__ x, int64_t r, bool live, int sub,
                                           int D, double (&t)[CPL]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = sub + k * LPR;
    t[k] = (live && c < D) ? (double)__builtin_nontemporal_load(x + r * D + c) : 0.0;
    s += t[k];
  }
  const double mean = group_sum<LPR>(s) / (double)D;
#pragma unroll
  for (int k = 0; k < CPL; ++k) t[k] = sub + k * LPR < D ? t[k] - mean : -(double)INFINITY;
  softmax_group<LPR, CPL>(t);
}

// ---- predict -----------------------------------------------------------------
// IsotonicRegression.predict of one class: clip to [x[0], x[n-1]], then SciPy
// interp1d's linear rule (searchsorted left, index clipped to [1, n-1]).
__device__ __forceinline__ double lookup(const double* tx, const double* ty, int n, double s) {
  if (n <= 0) return 0.0;
  if (n == 1) return ty[0];
  s = s < tx[0] ? tx[0] : s > tx[n - 1] ? tx[n - 1] : s;
  int lo = 0, hi = n;  // first index with tx[index] >= s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tx[mid] < s)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int i = lo < 1 ? 1 : lo > n - 1 ? n - 1 : lo;
  const double slope = (ty[i] - ty[i - 1]) / (tx[i] - tx[i - 1]);
  return slope * (s - tx[i - 1]) + ty[i - 1];
}

template <int LPR, int CPL, bool LDS>
__global__ __launch_bounds__(kThreads) void k_predict(
    const float* __restrict__ x, const double* __restrict__ thr_x,
    const double* __restrict__ thr_y, const int32_t* __restrict__ n_thr, int cap,
    const double* __restrict__ lp, float* __restrict__ probs, int D, int64_t B) {
  __shared__ double tab[LDS ? 2 * kLdsEntries : 1];
  constexpr int RPB = kThreads / LPR;
  const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const double* tx = thr_x;
  const double* ty = thr_y;
  if (LDS) {
    const int total = D * cap;  // <= kLdsEntries
    for (int e = threadIdx.x; e < total; e += kThreads) {
      if (e % cap < n_thr[e / cap]) {
        tab[e] = thr_x[e];
        tab[total + e] = thr_y[e];
      }
    }
    __syncthreads();
    tx = tab;
    ty = tab + total;
  }
  int nv[CPL];
  double lpv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = sub + k * LPR;
    nv[k] = c < D ? min(n_thr[c], cap) : 0;
    lpv[k] = c < D ? lp[c] : 0.0;
  }
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < B; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + grp;
    const bool live = r < B;
    double t[CPL];
    row_scores<LPR, CPL>(x, r, live, sub, D, t);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = sub + k * LPR;
      t[k] = c < D ? lookup(tx + (int64_t)c * cap, ty + (int64_t)c * cap, nv[k], t[k]) : 0.0;
      s += t[k];
    }
    s = group_sum<LPR>(s);
    // a row of zeros becomes NaN, as the reference's division leaves it
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      t[k] = sub + k * LPR < D ? log(t[k] / s + 1e-7) - lpv[k] : -(double)INFINITY;
    softmax_group<LPR, CPL>(t);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = sub + k * LPR;
      if (live && c < D) probs[r * D + c] = (float)t[k];
    }
  }
}

int rows_per_block(int D) { return D <= 16 ? kThreads : D <= 64 ? kThreads / 16 : kThreads / 64; }
int row_grid(int D, int64_t B) {
  const int64_t rpb = rows_per_block(D);
  return (int)std::min<int64_t>(1024, (B + rpb - 1) / rpb);
}

template <bool LDS>
void launch_predict(hipStream_t s, const float* x, const double* tx, const double* ty,
                    const int32_t* nt, int cap, const double* lp, float* probs, int D, int64_t B) {
  const dim3 g(row_grid(D, B)), t(kThreads);
  if (D <= 4)
    hipLaunchKernelGGL((k_predict<1, 4, LDS>), g, t, 0, s, x, tx, ty, nt, cap, lp, probs, D, B);
  else if (D <= 16)
    hipLaunchKernelGGL((k_predict<1, 16, LDS>), g, t, 0, s, x, tx, ty, nt, cap, lp, probs, D, B);
  else if (D <= 64)
    hipLaunchKernelGGL((k_predict<16, 4, LDS>), g, t, 0, s, x, tx, ty, nt, cap, lp, probs, D, B);
  else
    hipLaunchKernelGGL((k_predict<64, 4, LDS>), g, t, 0, s, x, tx, ty, nt, cap, lp, probs, D, B);
}

int check_shape(int32_t dim) {
  if (dim < 2) return CNF_ERR_DESC;
  if (dim > CNF_MAX_DIM) return CNF_ERR_UNSUPPORTED;
  return CNF_OK;
}

}  // namespace
}  // namespace cnf

extern "C" int cnf_pav_predict(const float* x, int32_t dim, int64_t B, const double* thr_x,
                               const double* thr_y, const int32_t* n_thr, int32_t cap,
                               const double* log_priors, float* probs, void* stream) {
  using namespace cnf;
  CNF_RANGE("cnf_pav_predict");
  const int st = check_shape(dim);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (cap < 1) return CNF_ERR_DESC;
  if (!thr_x || !thr_y || !n_thr || !log_priors || (B > 0 && (!x || !probs))) return CNF_ERR_NULL;
  if (mis4(x) || mis4(probs) || mis8(thr_x) || mis8(thr_y) || mis4(n_thr) || mis8(log_priors))
    return CNF_ERR_ALIGN;
  if (B == 0) return CNF_OK;
  const hipStream_t s = (hipStream_t)stream;
  if ((int64_t)dim * cap <= kLdsEntries)
    launch_predict<true>(s, x, thr_x, thr_y, n_thr, cap, log_priors, probs, dim, B);
  else
    launch_predict<false>(s, x, thr_x, thr_y, n_thr, cap, log_priors, probs, dim, B);
  return launch_status();
}
