// Temperature / MLR / vector / matrix scaling on the device (the reference's
// calibrators.py:57-205 and utils/ops.py:69-115): one fused pass evaluates the
// objective sum_r -log(softmax(t_r)[y_r] + 1e-7) of an affine map t = x.A + b
// of the logits and the raw sums its gradients are made of
// (cnf_scaling_loss_grad); a second entry point is the fused
// Calibrator.predict of the fitted map (cnf_scaling_predict).  include/cnf.h
// documents the layout of `sums`; the host forms the reference's formulas from
// them (cnf_hip/scaling.py, calibrators.py).
//
// Precision ("Scaling calibrators"): the logits are read as fp32
// and widened; the affine map, row maximum, exp, sum, log, the gradient terms
// and every sum over rows are float64.  SciPy's Newton-CG differences the
// gradient at a step below an fp32 ulp of T, and CG's line search stalls on
// fp32 row math, so nothing after the load is narrower than a double.
//
// Mechanism.  Scalar and diagonal kinds (k_scale_rows): LPR lanes share a row
// (1 lane for D <= 16, the row's values in its registers; 16 / 64 lanes for
// wider rows, coalesced column strides), each lane keeps float64 accumulators
// for its own columns over a grid-stride loop, and the block adds them with a
// fixed butterfly plus a four-wave LDS step.  Full kind (k_scale_full): a tile
// of 4096 / DP rows (DP: D padded to 16 / 32 / 64 / 128) is staged in LDS as
// fp32; phase 1 forms x @ W with each thread owning one output column of 16
// rows, phase 2 runs the row math with DP / 16 lanes per row and leaves
// g = p - onehot in LDS, phase 3 accumulates X^T G with each thread owning
// DP^2 / 256 words of the gradient for the whole launch.  Every block writes
// its float64 partial sums to the caller's workspace and k_scale_finish adds
// them in block order (one wave per word): no float atomics, no spin-wait, no
// allocation, no host sync; the grid depends on (kind, D, B) only, so two calls
// agree bitwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cnf_internal.h"

namespace cnf {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowBlocks = 1024;          // grid cap of k_scale_rows
constexpr int64_t kMaxRows = 1LL << 26;   // as cnf_metrics: sums of <= 2^26 terms
constexpr int kFullMaxDim = 128;          // full kind: W (128 KiB) stays L2-resident
constexpr int kTileElems = 4096;          // full kind: rows per tile * DP
enum Mode { kLoss = 0, kGrad = 1, kPredict = 2 };

// sum over the lanes whose index agrees modulo LO (LO = 1: the whole wave), in
// a fixed order; every lane of a class ends with the same bits
template <int LO>
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= LO; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
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

// t[k]: column sub + k * LPR of the row this lane group holds (-inf beyond D).
// On return t[k] = softmax(t)[column], formed as SciPy forms it:
// exp(t - max) / sum.
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

// The loss term and g = p - onehot of one row from its softmax p (in t, which
// g replaces when GRAD).  A label outside [0, D) turns both into NaN.  Returns
// the term (the same value in every lane of the group).
template <int LPR, int CPL, bool GRAD>
__device__ __forceinline__ double row_loss(double (&t)[CPL], int sub, int D, int64_t label) {
  const bool ok = label >= 0 && label < (int64_t)D;
  double py = 0.0;  // non-zero in at most one lane of the group
#pragma unroll
  for (int k = 0; k < CPL; ++k)
    if ((int64_t)(sub + k * LPR) == label) py = t[k];
  py = group_sum<LPR>(py);
  if (GRAD) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = sub + k * LPR;
      t[k] = !ok ? (double)NAN : (int64_t)c == label ? t[k] - 1.0 : t[k];
    }
  }
  return ok ? -log(py + 1e-7) : (double)NAN;
}

// The prior correction of Calibrator.predict on a row's softmax p (in t):
// softmax(log(p + 1e-7) - log_priors).
template <int LPR, int CPL>
__device__ __forceinline__ void prior_correct(double (&t)[CPL], const double (&lpv)[CPL], int sub,
                                              int D) {
#pragma unroll
  for (int k = 0; k < CPL; ++k)
    t[k] = sub + k * LPR < D ? log(t[k] + 1e-7) - lpv[k] : -(double)INFINITY;
  softmax_group<LPR, CPL>(t);
}

// ---- scalar and diagonal kinds ------------------------------------------
template <int KIND, int LPR, int CPL, int MODE>
__global__ __launch_bounds__(kThreads) void k_scale_rows(
    const float* __restrict__ x, const int64_t* __restrict__ y, const double* __restrict__ a,
    const double* __restrict__ b, const double* __restrict__ lp, double* __restrict__ part,
    float* __restrict__ probs, int D, int64_t B) {
  constexpr int RPB = kThreads / LPR;  // rows per block and pass
  const int sub = threadIdx.x % LPR;
  const int grp = threadIdx.x / LPR;
  double av[CPL], bv[CPL], lpv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = sub + k * LPR;
    av[k] = c < D ? (KIND == CNF_SCALE_SCALAR ? a[0] : a[c]) : 0.0;
    bv[k] = (c < D && b) ? b[c] : 0.0;
    lpv[k] = (MODE == kPredict && c < D) ? lp[c] : 0.0;
  }
  double loss = 0.0, gb[CPL], ga[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) gb[k] = ga[k] = 0.0;

  // the loop bound is uniform over the block: every lane takes part in the shuffles
  for (int64_t rb = (int64_t)blockIdx.x * RPB; rb < B; rb += (int64_t)gridDim.x * RPB) {
    const int64_t r = rb + grp;
    const bool live = r < B;
    float xv[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = sub + k * LPR;
      xv[k] = (live && c < D) ? __builtin_nontemporal_load(x + r * D + c) : 0.f;
    }
    double mean = 0.0;
    if (MODE == kPredict) {  // Calibrator.predict centres the row first
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < CPL; ++k) s += (double)xv[k];
      mean = group_sum<LPR>(s) / (double)D;
    }
    double t[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      t[k] = sub + k * LPR < D ? av[k] * ((double)xv[k] - mean) + bv[k] : -(double)INFINITY;
    softmax_group<LPR, CPL>(t);
    if (MODE == kPredict) {
      prior_correct<LPR, CPL>(t, lpv, sub, D);
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = sub + k * LPR;
        if (live && c < D) probs[r * D + c] = (float)t[k];
      }
    } else {
      const int64_t label = live ? y[r] : 0;
      const double term = row_loss<LPR, CPL, MODE == kGrad>(t, sub, D, label);
      if (live) {
        if (sub == 0) loss += term;
        if (MODE == kGrad) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            if (sub + k * LPR < D) {
              gb[k] += t[k];
              ga[KIND == CNF_SCALE_SCALAR ? 0 : k] += t[k] * (double)xv[k];
            }
          }
        }
      }
    }
  }
  if (MODE == kPredict) return;

  // block sums: a butterfly over the lanes that hold the same columns, then
  // the four waves in order
  __shared__ double red[kWaves][1 + 2 * CNF_MAX_DIM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int words = MODE == kGrad ? 1 + D + (KIND == CNF_SCALE_SCALAR ? 1 : D) : 1;
  {
    const double v = wave_sum<1>(loss);
    if (lane == 0) red[wave][0] = v;
  }
  if (MODE == kGrad) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = sub + k * LPR;
      const double v = wave_sum<LPR>(gb[k]);
      if (lane < LPR && c < D) red[wave][1 + c] = v;
      if (KIND == CNF_SCALE_DIAG) {
        const double w = wave_sum<LPR>(ga[k]);
        if (lane < LPR && c < D) red[wave][1 + D + c] = w;
      }
    }
    if (KIND == CNF_SCALE_SCALAR) {
      const double w = wave_sum<1>(ga[0]);
      if (lane == 0) red[wave][1 + D] = w;
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += kThreads)
    part[(int64_t)blockIdx.x * words + w] = ((red[0][w] + red[1][w]) + red[2][w]) + red[3][w];
}

// ---- full kind ------------------------------------------------------------
template <int DP, int MODE>
__global__ __launch_bounds__(kThreads) void k_scale_full(
    const float* __restrict__ x, const int64_t* __restrict__ y, const double* __restrict__ W,
    const double* __restrict__ b, const double* __restrict__ lp, double* __restrict__ part,
    float* __restrict__ probs, int D, int64_t B) {
  constexpr int TR = kTileElems / DP;   // rows per tile: 256 / 128 / 64 / 32
  constexpr int NG = kThreads / DP;     // thread groups of DP columns: 16 / 8 / 4 / 2
  constexpr int RPT = TR / NG;          // phase 1: rows per thread (16)
  constexpr int LPR = kThreads / TR;    // phase 2: lanes per row: 1 / 2 / 4 / 8
  constexpr int CPL = DP / LPR;         // phase 2: columns per lane (16)
  constexpr int IPT = DP / NG;          // phase 3: gradient rows per thread: 1 / 4 / 16 / 64
  constexpr int SX = DP + 1, SG = DP + 1;  // odd strides: no bank conflict at LPR = 1
  static_assert(RPT == 16 && CPL == 16, "tile shape");
  __shared__ float xs[TR * SX];
  __shared__ double gs[TR * SG];
  __shared__ double wsum[DP];
  __shared__ double red[kWaves];

  const int j = threadIdx.x % DP, ig = threadIdx.x / DP;  // phases 1 and 3
  const int sub = threadIdx.x % LPR, row = threadIdx.x / LPR;  // phase 2
  double bv[CPL], lpv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = sub + k * LPR;
    bv[k] = c < D ? b[c] : 0.0;
    lpv[k] = (MODE == kPredict && c < D) ? lp[c] : 0.0;
  }
  double loss = 0.0, gbacc = 0.0, gaacc[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) gaacc[k] = 0.0;

  for (int64_t r0 = (int64_t)blockIdx.x * TR; r0 < B; r0 += (int64_t)gridDim.x * TR) {
    // phase 0: the tile's rows as fp32, zero beyond B and D
    for (int idx = threadIdx.x; idx < TR * DP; idx += kThreads) {
      const int rr = idx / DP, c = idx % DP;
      const int64_t r = r0 + rr;
      xs[rr * SX + c] = (r < B && c < D) ? __builtin_nontemporal_load(x + r * D + c) : 0.f;
    }
    __syncthreads();

    // phase 1: x @ W, column j of rows ig * 16 .. ig * 16 + 15
    {
      double acc[RPT], ws = 0.0;
#pragma unroll
      for (int k = 0; k < RPT; ++k) acc[k] = 0.0;
      for (int i = 0; i < D; ++i) {
        const double w = j < D ? W[i * D + j] : 0.0;
        ws += w;
#pragma unroll
        for (int k = 0; k < RPT; ++k) acc[k] += (double)xs[(ig * RPT + k) * SX + i] * w;
      }
#pragma unroll
      for (int k = 0; k < RPT; ++k) gs[(ig * RPT + k) * SG + j] = acc[k];
      if (MODE == kPredict && ig == 0) wsum[j] = ws;
    }
    __syncthreads();

    // phase 2: the row math, LPR lanes per row
    {
      const int64_t r = r0 + row;
      const bool live = r < B;
      double mean = 0.0;
      if (MODE == kPredict) {  // (x - mean) @ W = x @ W - mean * colsum(W)
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) s += (double)xs[row * SX + sub + k * LPR];
        mean = group_sum<LPR>(s) / (double)D;
      }
      double t[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = sub + k * LPR;
        double v = gs[row * SG + c] + bv[k];
        if (MODE == kPredict) v -= mean * wsum[c];
        t[k] = c < D ? v : -(double)INFINITY;
      }
      softmax_group<LPR, CPL>(t);
      if (MODE == kPredict) {
        prior_correct<LPR, CPL>(t, lpv, sub, D);
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = sub + k * LPR;
          if (live && c < D) probs[r * D + c] = (float)t[k];
        }
      } else {
        const int64_t label = live ? y[r] : 0;
        const double term = row_loss<LPR, CPL, MODE == kGrad>(t, sub, D, label);
        if (live && sub == 0) loss += term;
        if (MODE == kGrad) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            const int c = sub + k * LPR;
            gs[row * SG + c] = (live && c < D) ? t[k] : 0.0;
          }
        }
      }
    }
    __syncthreads();

    // phase 3: X^T G, words (ig * IPT .. + IPT - 1, j); gb from the group ig == 0
    if (MODE == kGrad) {
      for (int rr = 0; rr < TR; ++rr) {
        const double g = gs[rr * SG + j];
        if (ig == 0) gbacc += g;
#pragma unroll
        for (int k = 0; k < IPT; ++k) gaacc[k] += (double)xs[rr * SX + ig * IPT + k] * g;
      }
      __syncthreads();  // the next tile overwrites xs and gs
    }
  }
  if (MODE == kPredict) return;

  const int words = MODE == kGrad ? 1 + D + D * D : 1;
  double* out = part + (int64_t)blockIdx.x * words;
  {
    const double v = wave_sum<1>(loss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
  if (MODE == kGrad && j < D) {
    if (ig == 0) out[1 + j] = gbacc;
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int i = ig * IPT + k;
      if (i < D) out[1 + D + i * D + j] = gaacc[k];
    }
  }
}

// sums[w] = partials[0][w] + partials[1][w] + ... : one wave per word, lane l
// adds blocks l, l + 64, ... in order, then a fixed butterfly
__global__ __launch_bounds__(kThreads) void k_scale_finish(const double* __restrict__ part,
                                                           int nblk, int words,
                                                           double* __restrict__ sums) {
  const int w = blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  double v = 0.0;
  if (w < words)
    for (int blk = lane; blk < nblk; blk += 64) v += part[(int64_t)blk * words + w];
  v = wave_sum<1>(v);
  if (w < words && lane == 0) sums[w] = v;
}

int check_shape(int32_t kind, int32_t dim) {
  if (kind != CNF_SCALE_SCALAR && kind != CNF_SCALE_DIAG && kind != CNF_SCALE_FULL)
    return CNF_ERR_DESC;
  if (dim < 2) return CNF_ERR_DESC;
  if (dim > (kind == CNF_SCALE_FULL ? kFullMaxDim : CNF_MAX_DIM)) return CNF_ERR_UNSUPPORTED;
  return CNF_OK;
}

int64_t grad_words(int32_t kind, int32_t dim) {
  const int64_t D = dim;
  return 1 + D + (kind == CNF_SCALE_SCALAR ? 1 : kind == CNF_SCALE_DIAG ? D : D * D);
}

int full_dp(int32_t dim) { return dim <= 16 ? 16 : dim <= 32 ? 32 : dim <= 64 ? 64 : 128; }

// rows per block and pass, and the grid: functions of (kind, D, B) only
int64_t rows_per_pass(int32_t kind, int32_t dim) {
  if (kind == CNF_SCALE_FULL) return kTileElems / full_dp(dim);
  return dim <= 16 ? kThreads : dim <= 64 ? kThreads / 16 : kThreads / 64;
}
int grid_cap(int32_t kind, int32_t dim) {
  if (kind != CNF_SCALE_FULL) return kRowBlocks;
  const int dp = full_dp(dim);  // fewer blocks as the per-block gradient grows
  return dp <= 32 ? 768 : dp == 64 ? 512 : 256;
}
int grid_blocks(int32_t kind, int32_t dim, int64_t B) {
  const int64_t rpb = rows_per_pass(kind, dim);
  return (int)std::min<int64_t>(grid_cap(kind, dim), (B + rpb - 1) / rpb);
}

template <int KIND, int MODE>
void launch_rows(int blocks, hipStream_t s, const float* x, const int64_t* y, const double* a,
                 const double* b, const double* lp, double* part, float* probs, int D, int64_t B) {
  const dim3 g(blocks), t(kThreads);
  if (D <= 4)
    hipLaunchKernelGGL((k_scale_rows<KIND, 1, 4, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs, D,
                       B);
  else if (D <= 16)
    hipLaunchKernelGGL((k_scale_rows<KIND, 1, 16, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs,
                       D, B);
  else if (D <= 64)
    hipLaunchKernelGGL((k_scale_rows<KIND, 16, 4, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs,
                       D, B);
  else
    hipLaunchKernelGGL((k_scale_rows<KIND, 64, 4, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs,
                       D, B);
}

template <int MODE>
void launch_full(int blocks, hipStream_t s, const float* x, const int64_t* y, const double* a,
                 const double* b, const double* lp, double* part, float* probs, int D, int64_t B) {
  const dim3 g(blocks), t(kThreads);
  switch (full_dp(D)) {
    case 16:
      hipLaunchKernelGGL((k_scale_full<16, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs, D, B);
      break;
    case 32:
      hipLaunchKernelGGL((k_scale_full<32, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs, D, B);
      break;
    case 64:
      hipLaunchKernelGGL((k_scale_full<64, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs, D, B);
      break;
    default:
      hipLaunchKernelGGL((k_scale_full<128, MODE>), g, t, 0, s, x, y, a, b, lp, part, probs, D, B);
  }
}

template <int MODE>
void launch(int32_t kind, int blocks, hipStream_t s, const float* x, const int64_t* y,
            const double* a, const double* b, const double* lp, double* part, float* probs, int D,
            int64_t B) {
  if (kind == CNF_SCALE_SCALAR)
    launch_rows<CNF_SCALE_SCALAR, MODE>(blocks, s, x, y, a, b, lp, part, probs, D, B);
  else if (kind == CNF_SCALE_DIAG)
    launch_rows<CNF_SCALE_DIAG, MODE>(blocks, s, x, y, a, b, lp, part, probs, D, B);
  else
    launch_full<MODE>(blocks, s, x, y, a, b, lp, part, probs, D, B);
}

}  // namespace
}  // namespace cnf

extern "C" int cnf_scaling_sums_words(int32_t kind, int32_t dim, int64_t* words) {
  using namespace cnf;
  if (!words) return CNF_ERR_NULL;
  const int st = check_shape(kind, dim);
  if (st != CNF_OK) return st;
  *words = grad_words(kind, dim);
  return CNF_OK;
}

extern "C" int cnf_scaling_workspace_bytes(int32_t kind, int32_t dim, int64_t B, size_t* bytes) {
  using namespace cnf;
  if (!bytes) return CNF_ERR_NULL;
  const int st = check_shape(kind, dim);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  *bytes = (size_t)grid_blocks(kind, dim, B) * (size_t)grad_words(kind, dim) * sizeof(double);
  return CNF_OK;
}

extern "C" int cnf_scaling_loss_grad(const float* x, const int64_t* y, int32_t kind, int32_t dim,
                                     const double* a, const double* b, int32_t want_grad,
                                     int64_t B, double* sums, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  using namespace cnf;
  CNF_RANGE("cnf_scaling_loss_grad");
  const int st = check_shape(kind, dim);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!sums || !a || (!b && kind != CNF_SCALE_SCALAR) || (B > 0 && (!x || !y)))
    return CNF_ERR_NULL;
  const int64_t words = want_grad ? grad_words(kind, dim) : 1;
  const int blocks = grid_blocks(kind, dim, B);
  if (B > 0 && (!workspace || workspace_bytes < (size_t)blocks * words * sizeof(double)))
    return CNF_ERR_NULL;
  if (mis4(x) || mis8(y) || mis8(a) || mis8(b) || mis8(sums) || mis8(workspace))
    return CNF_ERR_ALIGN;
  const hipStream_t s = (hipStream_t)stream;
  if (B == 0)  // empty sums; a memset node, no kernel
    return hip_status(hipMemsetAsync(sums, 0, (size_t)words * sizeof(double), s));
  double* part = static_cast<double*>(workspace);
  if (want_grad)
    launch<kGrad>(kind, blocks, s, x, y, a, b, nullptr, part, nullptr, dim, B);
  else
    launch<kLoss>(kind, blocks, s, x, y, a, b, nullptr, part, nullptr, dim, B);
  const int st2 = launch_status();
  if (st2 != CNF_OK) return st2;
  hipLaunchKernelGGL(k_scale_finish, dim3((unsigned)((words + kWaves - 1) / kWaves)),
                     dim3(kThreads), 0, s, part, blocks, (int)words, sums);
  return launch_status();
}

extern "C" int cnf_scaling_predict(const float* x, int32_t kind, int32_t dim, const double* a,
                                   const double* b, const double* log_priors, float* probs,
                                   int64_t B, void* stream) {
  using namespace cnf;
  CNF_RANGE("cnf_scaling_predict");
  const int st = check_shape(kind, dim);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!a || !log_priors || (!b && kind != CNF_SCALE_SCALAR) || (B > 0 && (!x || !probs)))
    return CNF_ERR_NULL;
  if (mis4(x) || mis4(probs) || mis8(a) || mis8(b) || mis8(log_priors)) return CNF_ERR_ALIGN;
  if (B == 0) return CNF_OK;
  launch<kPredict>(kind, grid_blocks(kind, dim, B), (hipStream_t)stream, x, nullptr, a, b,
                   log_priors, nullptr, probs, dim, B);
  return launch_status();
}
