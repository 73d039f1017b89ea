// Radial flows (the reference's RadialLayer, flows/flows.py:168-193) as fused
// HIP kernels: forward (+ loss terms), the hand-derived reverse mode (+ fused
// loss seed), and the calibrator's predict (centring, the stack, both softmaxes
// and the prior correction in one pass) with its score variant (the predict
// ending in cnf_metrics' record, cnf_score.h), all fp32.  The layer's log-det
// is the reference's constant log(1) = 0: no kernel computes or stores one.
//
// Geometry, grid caps, workspace plan, argument checks, shape dispatch and the
// lane helpers are cnf_rowflow.h's, shared with cnf_planar.hip.  The kernel
// bodies -- tile staging, the predict body, the reverse-mode frame, the finish
// kernel's record add -- are this file's own text, as the planar ones are
// theirs: shared as helpers they compile to different code.
//
// Rows: one lane per row for D <= 16 (the row in registers), 16 lanes per row
// for D <= 64, 64 lanes per row above (column c of a row sits in lane c % LPR,
// slot c / LPR; the norm and the dot product end in an xor butterfly over the
// row's lanes).  Every kernel walks the batch in a grid-stride loop under a
// fixed grid cap, so the order of every sum depends on (D, L, B) only.  The
// one-lane rows of the forward and predict kernels move through an LDS tile as
// coalesced sweeps.
//
// Per-layer constants.  k_radial_prep (L blocks) writes, per layer,
//   [z0[DP] | a, sp, beta, sigmoid(b), 0, 0, 0, 0]          DP = LPR * CPL
// with sp = log1p(exp(b)) and beta = sp - a into the caller's workspace; the
// row kernels and the finish step read that one record.
//
// Reverse mode.  The forward sweep keeps one r = ||x - z0|| per (row, layer):
// in registers up to kRegL layers, in an [L][B] tape in the workspace above.
// Because 1 + beta h = (r + sp) / (a + r), the backward sweep rebuilds
// d_l = (z_l - z0_l) (a + r) / (r + sp) and x_l = z0_l + d_l; r + sp > 0 for
// every finite b.  Each inversion multiplies the rebuilt row's error by
// (a + r) / (r + sp), so above kRegL layers the row is run forward again from
// the input every kRebuild layers.
// The D + 2 row sums per layer (sum g_d [D], g_beta, sum g_r) live in per-lane
// accumulators over the whole grid-stride loop when one lane holds a row and L <= kRegL (one wave sum at the end); otherwise each pass
// ends in a wave sum per word that one fixed lane adds into the wave's record
// (LDS, or the workspace when 4 records exceed 48 KB).  Block (or wave) records
// go to the workspace; k_radial_finish adds them in index order, applies the
// chain rule through beta = log1p(exp(b)) - a and writes the flat gradient
// (z0, a, b per layer).  No float atomics, no inter-block dependency, no
// spin-wait, no data-dependent loop, no allocation, no host sync; every barrier
// sits under block-uniform bounds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cnf_internal.h"
#include "cnf_rowflow.h"
#include "cnf_score.h"
#include "cnf_valu_io.h"

namespace cnf {
namespace {

using namespace rowflow;
using valu::wave_sum_dpp63;

constexpr int kMaxL = CNF_RADIAL_MAX_LAYERS;
constexpr int kRebuild = 16;  // workspace-tape reverse mode: longest chain of layer inversions

struct Ptrs {
  const float* p[3 * kMaxL];
};

// per layer: the constant record [z0 | 8 scalars], D + 2 row sums
Geo radial_geometry(int D, int L) { return geometry(D, L, padded_dim(D) + 8, D + 2); }
// reverse mode: the tape in registers up to kRegL layers; per-lane accumulators
// on top of it for every one-lane row
constexpr BwdVariant radial_bwd_variant(int lpr, int /*cpl*/, int L) {
  const bool regt = L <= kRegL;
  return {regt, regt && lpr == 1};
}
constexpr RowFamily kFamily{kMaxL, radial_geometry, radial_bwd_variant};

// ---- per-layer constants --------------------------------------------------

// The one evaluation of the reference's scalars (flows/flows.py:186):
// [a, sp = log1p(exp(b)), beta = -a + sp, sigmoid(b)].
__global__ __launch_bounds__(64) void k_radial_prep(Ptrs P, float* __restrict__ blob, int D, int dp,
                                                    int cs) {
  const int l = blockIdx.x, t = threadIdx.x;
  const float* z0 = P.p[3 * l];
  float* o = blob + (size_t)l * cs;
  for (int j = t; j < dp; j += 64) o[j] = j < D ? z0[j] : 0.f;
  if (t == 0) {
    const float a = P.p[3 * l + 1][0];
    const float b = P.p[3 * l + 2][0];
    const float sp = log1pf(expf(b));
    o[dp] = a;
    o[dp + 1] = sp;
    o[dp + 2] = -a + sp;
    o[dp + 3] = 1.f / (1.f + expf(-b));
    o[dp + 4] = 0.f;
    o[dp + 5] = 0.f;
    o[dp + 6] = 0.f;
    o[dp + 7] = 0.f;
  }
}

// ---- row steps --------------------------------------------------------------

// One layer forward on the row's registers; returns r = ||x - z0||.  Padding
// columns hold 0 in xv and in z0, so they add nothing to the norm and stay 0.
template <int LPR, int CPL>
__device__ __forceinline__ float radial_step(float* xv, const float* __restrict__ cb, int gl) {
  constexpr int DP = LPR * CPL;
  float d[CPL];
  float r2 = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    d[k] = xv[k] - cb[gl + LPR * k];
    r2 = fmaf(d[k], d[k], r2);
  }
  const float r = sqrtf(row_sum<LPR>(r2));
  const float h = 1.f / (cb[DP] + r);
  const float bh = cb[DP + 2] * h;
#pragma unroll
  for (int k = 0; k < CPL; ++k) xv[k] = fmaf(bh, d[k], xv[k]);
  return r;
}

// the log-det is 0, so the loss is its cross-entropy term
__device__ __forceinline__ float loss_term(int kind, float lpy, bool yok) {
  const float ce = kind == CNF_LOSS_CAL ? -logf(expf(lpy) + 1e-7f) : -lpy;
  return yok ? ce : NAN;
}

// ---- forward ----------------------------------------------------------------

template <int LPR, int CPL>
__global__ __launch_bounds__(kThreads) void k_radial_fwd(
    const float* __restrict__ x, const float* __restrict__ blob, int D, int L, int cs, int64_t B,
    float* __restrict__ z, float* __restrict__ z_all, const int64_t* __restrict__ y, int kind,
    float* __restrict__ part) {
  constexpr int RPB = kThreads / LPR;
  // One lane per row (D == CPL): the block's rows -- one contiguous run of
  // nrows * D floats -- go through an LDS tile (odd row stride TS: no bank
  // conflicts) and move as coalesced 4-byte-per-lane sweeps.  Every loop bound
  // below is block-uniform, so every thread reaches every barrier.
  constexpr bool kStage = LPR == 1;
  constexpr int TS = CPL | 1;
  __shared__ float tile[kStage ? kThreads * TS : 1];
  __shared__ float red[kWaves * 4];
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR;
  float t0 = 0.f;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < B; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + gi;
    const bool valid = row < B;
    const int nrows = B - base < RPB ? (int)(B - base) : RPB;
    float xv[CPL];
    auto tile_out = [&](float* __restrict__ dst) {  // dst: the block's first row
#pragma unroll
      for (int k = 0; k < CPL; ++k) tile[tid * TS + k] = xv[k];
      __syncthreads();
      for (int i = tid; i < nrows * CPL; i += kThreads) {
        const int r = i / CPL;
        dst[i] = tile[r * TS + (i - r * CPL)];
      }
      __syncthreads();
    };
    if constexpr (kStage) {
      const float* __restrict__ src = x + base * D;
      for (int i = tid; i < nrows * CPL; i += kThreads) {
        const int r = i / CPL;
        tile[r * TS + (i - r * CPL)] = src[i];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CPL; ++k) xv[k] = valid ? tile[tid * TS + k] : 0.f;
      __syncthreads();
    } else {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        xv[k] = (valid && c < D) ? x[row * D + c] : 0.f;
      }
    }
    for (int l = 0; l < L; ++l) {
      radial_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl);
      if constexpr (kStage) {
        if (z_all) tile_out(z_all + ((int64_t)l * B + base) * D);
      } else if (z_all && valid) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int c = gl + LPR * k;
          if (c < D) z_all[((int64_t)l * B + row) * D + c] = xv[k];
        }
      }
    }
    if constexpr (kStage) {
      if (z) tile_out(z + base * D);
    } else if (z && valid) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        if (c < D) z[row * D + c] = xv[k];
      }
    }
    if (y) {
      const int64_t yy = valid ? y[row] : 0;
      float m, lse, lpy;
      row_softmax<LPR, CPL>(xv, gl, D, yy, m, lse, lpy);
      const float ce = loss_term(kind, lpy, yy >= 0 && yy < D);
      if (valid && gl == 0) t0 += ce;
    }
  }
  if (part) {  // block-uniform
    t0 = wave_sum_dpp63(t0);
    if ((tid & 63) == 63) red[tid >> 6] = t0;
    __syncthreads();
    if (tid < 4) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += red[w];
      // (loss, ce, log-det, pad): loss == ce, the log-det term is 0
      part[(size_t)blockIdx.x * 4 + tid] = tid < 2 ? s : 0.f;
    }
  }
}

// ---- predict ------------------------------------------------------------------

// Calibrator.predict of a radial flow calibrator (calibrators.py:40-44,
// 330-353), the row in registers from load to store: centre on the mean of the
// D real columns, run the stack, p = softmax(z), then
// softmax(log(p + 1e-7) - log_priors).  Padding columns (c >= D) hold 0 through
// the stack (their z0 is 0) and enter no mean, norm, maximum or sum.  Same
// grid, tile and barriers as k_radial_fwd.  SCORE: the scoring epilogue of
// cnf_score.h takes the fp32 probabilities in place of the store phase.
template <int LPR, int CPL, bool SCORE>
__global__ __launch_bounds__(kThreads) void k_radial_predict(
    const float* __restrict__ x, const float* __restrict__ blob, const float* __restrict__ lp,
    int D, int L, int cs, int64_t B, float* __restrict__ probs, score::Args sc) {
  constexpr int RPB = kThreads / LPR;
  constexpr bool kStage = LPR == 1;
  constexpr int TS = CPL | 1;
  __shared__ float tile[kStage ? kThreads * TS : 1];
  __shared__ long long rec[SCORE ? score::kRecWords : 1];
  score::Acc acc;
  if constexpr (SCORE) score::init(rec, sc.bins);
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR;
  float lpv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = gl + LPR * k;
    lpv[k] = c < D ? lp[c] : 0.f;
  }
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < B; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + gi;
    const bool valid = row < B;
    const int nrows = B - base < RPB ? (int)(B - base) : RPB;
    float xv[CPL];
    if constexpr (kStage) {
      const float* __restrict__ src = x + base * D;
      for (int i = tid; i < nrows * CPL; i += kThreads) {
        const int r = i / CPL;
        tile[r * TS + (i - r * CPL)] = src[i];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < CPL; ++k) xv[k] = valid ? tile[tid * TS + k] : 0.f;
      __syncthreads();
    } else {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        xv[k] = (valid && c < D) ? x[row * D + c] : 0.f;
      }
    }
    // centre
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (gl + LPR * k < D) s += xv[k];
    const float mu = row_sum<LPR>(s) / (float)D;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (gl + LPR * k < D) xv[k] -= mu;
    for (int l = 0; l < L; ++l) radial_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl);
    // p = softmax(z)
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (gl + LPR * k < D) m = fmaxf(m, xv[k]);
    m = row_max<LPR>(m);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (gl + LPR * k < D) se += expf(xv[k] - m);
    const float lse = logf(row_sum<LPR>(se));
    // q = log(p + 1e-7) - log_priors, probs = softmax(q)
    float m2 = -INFINITY;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float p = expf(xv[k] - m - lse);
      xv[k] = logf(p + 1e-7f) - lpv[k];
      if (gl + LPR * k < D) m2 = fmaxf(m2, xv[k]);
    }
    m2 = row_max<LPR>(m2);
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      xv[k] = expf(xv[k] - m2);
      if (gl + LPR * k < D) s2 += xv[k];
    }
    s2 = row_sum<LPR>(s2);
#pragma unroll
    for (int k = 0; k < CPL; ++k) xv[k] = xv[k] / s2;
    if constexpr (SCORE) {
      score::row<LPR, CPL>(xv, gl, D, valid ? sc.y[row] : -1, valid, sc.bins, sc.e, rec, acc);
    } else if constexpr (kStage) {
      float* __restrict__ dst = probs + base * D;
#pragma unroll
      for (int k = 0; k < CPL; ++k) tile[tid * TS + k] = xv[k];
      __syncthreads();
      for (int i = tid; i < nrows * CPL; i += kThreads) {
        const int r = i / CPL;
        dst[i] = tile[r * TS + (i - r * CPL)];
      }
      __syncthreads();
    } else if (valid) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        if (c < D) probs[row * D + c] = xv[k];
      }
    }
  }
  if constexpr (SCORE) score::flush(rec, sc.bins, acc, sc.record);
}

// ---- reverse mode -------------------------------------------------------------

struct BwdArgs {
  const float* x;
  const float* blob;
  const int64_t* y;     // non-null: the fused loss seeds the sweep
  const float* gz;      // upstream gradients (y == null), each may be null
  const float* gz_all;
  float* dx;
  float* part;          // block records (wave records when gacc)
  float* tape;          // [L][B] when L > kRegL
  int64_t B;
  int D, L, cs, ps, pw, gacc, kind;
  float gscale;
};

// Backward through layer l.  In: xv = z_l, g = gradient at z_l, r.  Out: xv =
// x_l, g = gradient at x_l; con[] = this row's CPL + 2 contributions
// [g_d | h s, g_r].  A row past the batch contributes exact zeros.
template <int LPR, int CPL>
__device__ __forceinline__ void radial_back(float* xv, float* g, float r, bool valid,
                                            const float* __restrict__ cb, int gl, float* con) {
  constexpr int DP = LPR * CPL;
  const float a = cb[DP], sp = cb[DP + 1], beta = cb[DP + 2];
  const float ar = a + r;
  const float back = ar / (r + sp);  // 1 / (1 + beta h)
  const float h = 1.f / ar;
  float d[CPL];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const float z0 = cb[gl + LPR * k];
    d[k] = (xv[k] - z0) * back;
    xv[k] = z0 + d[k];
    s = fmaf(g[k], d[k], s);
  }
  s = row_sum<LPR>(s);
  const float hs = h * s;
  const float gr = -h * beta * hs;
  const float gq = r != 0.f ? gr / r : 0.f;  // torch's norm backward: 0 at r == 0
  const float bh = beta * h;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const float gd = fmaf(gq, d[k], bh * g[k]);
    con[k] = valid ? gd : 0.f;
    g[k] += gd;
  }
  con[CPL] = valid ? hs : 0.f;
  con[CPL + 1] = valid ? gr : 0.f;
}

// Add one row pass's contributions of layer l into the wave's record: a wave
// sum per word, added by one fixed lane (so the order is fixed).
template <int LPR, int CPL>
__device__ __forceinline__ void record_add(float* rec, const float* con, int gl, int lane, int D) {
  if constexpr (LPR == 1) {
#pragma unroll
    for (int i = 0; i < CPL + 2; ++i) {
      const float v = wave_sum_dpp63(con[i]);
      if (lane == 63) rec[i] += v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float a = col_sum<LPR>(con[k]);
      const int c = gl + LPR * k;
      if (lane < LPR && c < D) rec[c] += a;
    }
    const float gb = col_sum<LPR>(con[CPL]);
    const float gr = col_sum<LPR>(con[CPL + 1]);
    if (lane == 0) {
      rec[D] += gb;
      rec[D + 1] += gr;
    }
  }
}

template <int LPR, int CPL, bool REGT, bool REGA>
__global__ __launch_bounds__(kThreads) void k_radial_bwd(BwdArgs A) {
  constexpr int RPB = kThreads / LPR;
  constexpr int NW = CPL + 2;
  extern __shared__ float sm[];
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR, lane = tid & 63, wave = tid >> 6;
  const int D = A.D, L = A.L, cs = A.cs, ps = A.ps, pw = A.pw;
  const int64_t B = A.B;
  const float* __restrict__ blob = A.blob;
  float* rec;  // this wave's record
  if (!A.gacc) {
    for (int i = tid; i < kWaves * pw; i += kThreads) sm[i] = 0.f;
    __syncthreads();
    rec = sm + wave * pw;
  } else {
    rec = A.part + ((size_t)blockIdx.x * kWaves + wave) * pw;  // zeroed by the host side
  }
  float racc[REGA ? kRegL * NW : 1];
#pragma unroll
  for (int i = 0; i < (REGA ? kRegL * NW : 1); ++i) racc[i] = 0.f;
  float t0 = 0.f;

  for (int64_t base = (int64_t)blockIdx.x * RPB; base < B; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + gi;
    const bool valid = row < B;
    float xv[CPL], g[CPL], con[NW];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = gl + LPR * k;
      xv[k] = (valid && c < D) ? A.x[row * D + c] : 0.f;
    }
    float rt[REGT ? kRegL : 1];
    if constexpr (REGT) {
#pragma unroll
      for (int l = 0; l < kRegL; ++l)
        if (l < L) rt[l] = radial_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl);
    } else {
      for (int l = 0; l < L; ++l) {
        const float r = radial_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl);
        if (valid && gl == 0) A.tape[(int64_t)l * B + row] = r;
      }
    }
    // seed
    if (A.y) {
      const int64_t yy = valid ? A.y[row] : 0;
      const bool yok = yy >= 0 && yy < D;
      float m, lse, lpy;
      row_softmax<LPR, CPL>(xv, gl, D, yy, m, lse, lpy);
      const float ce = loss_term(A.kind, lpy, yok);
      if (valid && gl == 0) t0 += ce;
      float coef = 1.f;
      if (A.kind == CNF_LOSS_CAL) {
        const float py = expf(lpy);
        coef = py / (py + 1e-7f);
      }
      coef *= A.gscale;
      if (!yok) coef = NAN;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        const float p = expf(xv[k] - m - lse);
        g[k] = (valid && c < D) ? coef * (p - (c == yy ? 1.f : 0.f)) : 0.f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        float v = 0.f;
        if (valid && c < D) {
          if (A.gz) v = A.gz[row * D + c];
          if (A.gz_all) v += A.gz_all[((int64_t)(L - 1) * B + row) * D + c];
        }
        g[k] = v;
      }
    }
    // backward sweep
    if constexpr (REGT) {
#pragma unroll
      for (int l = kRegL - 1; l >= 0; --l) {
        if (l < L) {
          radial_back<LPR, CPL>(xv, g, rt[l], valid, blob + (size_t)l * cs, gl, con);
          if constexpr (REGA) {
#pragma unroll
            for (int i = 0; i < NW; ++i) racc[l * NW + i] += con[i];
          } else {
            record_add<LPR, CPL>(rec + l * ps, con, gl, lane, D);
          }
          if (l > 0 && A.gz_all && valid) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
              const int c = gl + LPR * k;
              if (c < D) g[k] += A.gz_all[((int64_t)(l - 1) * B + row) * D + c];
            }
          }
        }
      }
    } else {
      for (int l = L - 1; l >= 0; --l) {
        float r = 0.f;
        if (valid && gl == 0) r = A.tape[(int64_t)l * B + row];  // the lane that wrote it
        r = __shfl(r, lane - gl);
        radial_back<LPR, CPL>(xv, g, r, valid, blob + (size_t)l * cs, gl, con);
        record_add<LPR, CPL>(rec + l * ps, con, gl, lane, D);
        if (l > 0 && A.gz_all && valid) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            const int c = gl + LPR * k;
            if (c < D) g[k] += A.gz_all[((int64_t)(l - 1) * B + row) * D + c];
          }
        }
        // Inverting a layer multiplies the error of the rebuilt row by
        // 1 / (1 + beta h) >= 1 where the layer contracts, so a deep
        // contracting stack loses the early layers' inputs (2e-3 absolute
        // after 64 layers at D = 3).  Every kRebuild layers the row is run
        // forward again from the input instead: the chain of inversions stays
        // at most kRebuild long.  Block-uniform bounds.
        if (l > 0 && l % kRebuild == 0) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            const int c = gl + LPR * k;
            xv[k] = (valid && c < D) ? A.x[row * D + c] : 0.f;
          }
          for (int j = 0; j < l; ++j) radial_step<LPR, CPL>(xv, blob + (size_t)j * cs, gl);
        }
      }
    }
    if (A.dx && valid) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int c = gl + LPR * k;
        if (c < D) A.dx[row * D + c] = g[k];
      }
    }
  }

  if constexpr (REGA) {  // LPR == 1, record in LDS, ps == NW
#pragma unroll
    for (int l = 0; l < kRegL; ++l) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const float v = wave_sum_dpp63(racc[l * NW + i]);
        if (lane == 63 && l < L) rec[l * NW + i] = v;
      }
    }
  }
  t0 = wave_sum_dpp63(t0);
  if (lane == 63) {
    rec[L * ps] = t0;      // loss
    rec[L * ps + 1] = t0;  // ce: the same sum, the log-det being 0
    rec[L * ps + 2] = 0.f;
    rec[L * ps + 3] = 0.f;
  }
  if (!A.gacc) {
    __syncthreads();
    float* out = A.part + (size_t)blockIdx.x * pw;
    for (int i = tid; i < pw; i += kThreads) {
      float s = sm[i];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) s += sm[w * pw + i];
      out[i] = s;
    }
  }
}

// ---- finish -------------------------------------------------------------------

// One block.  Adds `units` records of `pw` words in index order (a thread owns
// a contiguous run of units of one word; the runs are added in run order),
// writes the three loss terms, then applies the chain rule per layer
//   dL/dz0 = -sum g_d,  dL/da = sum g_r - g_beta,  dL/db = g_beta sigmoid(b)
// and writes the flat gradient.
__global__ __launch_bounds__(kFinThreads) void k_radial_finish(
    const float* __restrict__ part, int units, int pw, int nsum, float* __restrict__ sums,
    float* __restrict__ terms, float* __restrict__ grads, const float* __restrict__ blob, int D,
    int L, int dp, int cs) {
  __shared__ float red[kFinThreads];
  const int t = threadIdx.x;
  int wt = 4;
  while (wt < 64 && wt < pw) wt <<= 1;
  const int ug = kFinThreads / wt;
  const int wi = t % wt, gi = t / wt;
  const int chunk = (units + ug - 1) / ug;
  for (int w0 = 0; w0 < pw; w0 += wt) {
    const int w = w0 + wi;
    float s = 0.f;
    if (w < pw) {
      const int u0 = gi * chunk;
      const int u1 = u0 + chunk < units ? u0 + chunk : units;
#pragma unroll 8
      for (int u = u0; u < u1; ++u) s += part[(size_t)u * pw + w];
    }
    red[t] = s;
    __syncthreads();
    if (t < wt && w < pw) {
      float a = 0.f;
      for (int k = 0; k < ug; ++k) a += red[k * wt + t];
      if (w < nsum) {
        sums[w] = a;
      } else if (terms && w < nsum + 3) {
        terms[w - nsum] = a;
      }
    }
    __syncthreads();
  }
  if (!grads) return;  // block-uniform
  __syncthreads();
  const int ps = D + 2;
  for (int i = t; i < L * ps; i += kFinThreads) {
    const int l = i / ps, j = i - l * ps;
    const float* S = sums + (size_t)l * ps;
    float v;
    if (j < D) {
      v = -S[j];
    } else if (j == D) {
      v = S[D + 1] - S[D];
    } else {
      v = S[D] * blob[(size_t)l * cs + dp + 3];
    }
    grads[i] = v;
  }
}

// ---- launches -------------------------------------------------------------------

// What cnf_rowflow.h's launch layer asks of a family.
struct Radial {
  using Table = Ptrs;
  using Args = BwdArgs;
  static constexpr bool kLdScalar = false;  // no log-det at all
  static const RowFamily& family() { return kFamily; }
  static constexpr int grad_floats(int D, int = 0) { return D + 2; }  // z0, a, b
  static int8_t* kinds(Ptrs&) { return nullptr; }

  static void prep(const Ptrs& P, const Geo& g, int D, int L, float* blob, bool, hipStream_t s) {
    hipLaunchKernelGGL(k_radial_prep, dim3(L), dim3(64), 0, s, P, blob, D, g.dp, g.cs);
  }

  template <int LPR, int CPL>
  static void fwd(int blocks, const FwdCall& c, const Geo& g, const float* blob, float* part) {
    hipLaunchKernelGGL((k_radial_fwd<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x, blob,
                       c.D, c.L, g.cs, c.B, c.z, c.z_all, c.y, c.kind, part);
  }

  template <int LPR, int CPL>
  static void predict(int blocks, const PredictCall& c, const Geo& g, const float* blob,
                      const score::Args* sc) {
    if (sc) {
      hipLaunchKernelGGL((k_radial_predict<LPR, CPL, true>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, (float*)nullptr, *sc);
    } else {
      hipLaunchKernelGGL((k_radial_predict<LPR, CPL, false>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, c.probs, score::Args{});
    }
  }

  template <int LPR, int CPL>
  static void bwd(int blocks, size_t lds, hipStream_t s, const BwdArgs& a) {
    if (!radial_bwd_variant(LPR, CPL, a.L).regt) {
      hipLaunchKernelGGL((k_radial_bwd<LPR, CPL, false, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
      return;
    }
    // rega depends on the depth through regt alone: the geometry's answer at kRegL
    if constexpr (radial_bwd_variant(LPR, CPL, kRegL).rega) {
      hipLaunchKernelGGL((k_radial_bwd<LPR, CPL, true, true>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
    } else {
      hipLaunchKernelGGL((k_radial_bwd<LPR, CPL, true, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
    }
  }

  static void fill(BwdArgs& a, const BwdCall&, float* tape) { a.tape = tape; }

  static void finish(const Finish& f, const Ptrs&, int D, int L, const Geo& g, const BwdCall*,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_radial_finish, dim3(1), dim3(kFinThreads), 0, s, f.part, f.units, f.pw,
                       f.nsum, f.sums, f.terms, f.grads, f.blob, D, L, g.dp, g.cs);
  }
};

}  // namespace
}  // namespace cnf

extern "C" int cnf_radial_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats) {
  return cnf::rowflow::param_count(cnf::kFamily, cnf::Radial::grad_floats, dim, n_layers, n_floats);
}

extern "C" int cnf_radial_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B,
                                          size_t* bytes) {
  return cnf::rowflow::workspace_bytes(cnf::kFamily, dim, n_layers, B, bytes);
}

extern "C" int cnf_radial_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]) {
  return cnf::rowflow::launch_plan(cnf::kFamily, dim, n_layers, B, out);
}

extern "C" int cnf_radial_forward(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, float* z, float* z_all, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_radial_forward");
  return cnf::rowflow::run_forward<cnf::Radial>({dim, n_layers, params, x, nullptr, 0, 0.f, z,
                                                 nullptr, z_all, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false,
                                                 false});
}

extern "C" int cnf_radial_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                                       const float* x, const int64_t* y, int32_t loss_kind,
                                       float* z, float* loss_terms, int64_t B, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_radial_forward_loss");
  return cnf::rowflow::run_forward<cnf::Radial>({dim, n_layers, params, x, y, loss_kind, 0.f, z,
                                                 nullptr, nullptr, loss_terms, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true,
                                                 false});
}

extern "C" int cnf_radial_predict(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, const float* log_priors, float* probs, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_radial_predict");
  return cnf::rowflow::run_predict<cnf::Radial>({dim, n_layers, params, x, log_priors, probs,
                                                 nullptr, nullptr, 0, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false});
}

extern "C" int cnf_radial_score(int32_t dim, int32_t n_layers, const float* const* params,
                                const float* x, const float* log_priors, const int64_t* y,
                                int32_t bins, int64_t* record, int64_t B, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_radial_score");
  return cnf::rowflow::run_predict<cnf::Radial>({dim, n_layers, params, x, log_priors, nullptr,
                                                 nullptr, y, bins, record, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true});
}

extern "C" int cnf_radial_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                              const float* x, const float* gz, const float* gz_all, float* grads,
                              float* dx, int64_t B, void* workspace, size_t workspace_bytes,
                              void* stream) {
  CNF_RANGE("cnf_radial_vjp");
  return cnf::rowflow::run_backward<cnf::Radial>({dim, n_layers, params, x, nullptr, 0, 0.f, 1.f,
                                                  gz, gz_all, nullptr, nullptr, grads, dx, B,
                                                  workspace, workspace_bytes, (hipStream_t)stream,
                                                  false});
}

extern "C" int cnf_radial_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                                   const float* x, const int64_t* y, int32_t loss_kind,
                                   float grad_scale, float* loss_terms, float* grads, float* dx,
                                   int64_t B, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  CNF_RANGE("cnf_radial_loss_vjp");
  return cnf::rowflow::run_backward<cnf::Radial>({dim, n_layers, params, x, y, loss_kind, 0.f,
                                                  grad_scale, nullptr, nullptr, nullptr, loss_terms,
                                                  grads, dx, B, workspace, workspace_bytes,
                                                  (hipStream_t)stream, true});
}
