// Affine-constant flows (the reference's AffineConstantLayer, flows/flows.py:
// 40-65) as fused HIP kernels: forward and inverse (+ the one-number log-det,
// + loss terms), the hand-derived reverse mode of the forward (+ fused loss
// seed), and the calibrator's predict with its score variant (cnf_score.h),
// all fp32.
//
// Geometry, grid caps, workspace plan, argument checks, shape dispatch and the
// lane helpers are cnf_rowflow.h's, shared with cnf_planar.hip and
// cnf_radial.hip; the kernel bodies are this file's own text, as theirs are
// (DESIGN.md 7h).  Rows sit in lanes as in the siblings: one lane per row for
// D <= 16, 16 lanes for D <= 64, 64 above; every kernel walks the batch in a
// grid-stride loop under a fixed grid cap, so the order of every sum depends
// on (D, L, B) only.
//
// Per-layer constants.  k_affine_prep (one block) writes, per step k of the
// direction (layer k forward, layer L-1-k inverse),
//   [e[DP] | t[DP] | ld_k, ld_total (record 0 only), 0 x 6]      DP = LPR * CPL
// with e = exp(s) (exp(-s) inverse) and ld_k = sum_d s (sum_d -s): an fp32 sum
// over d, then ld_total = 0 + ld_0 + ld_1 + ... in step order, as Flow.forward
// / Flow.backward accumulate it.  The log-det is one number per call: no row
// kernel computes it.  Padding columns hold e = t = 0 and stay 0.
//
// A layer is applied as torch applies it -- a rounded product, then a rounded
// sum (x * e + t), or a rounded difference, then a rounded product
// ((z - t) * e) -- layer after layer in registers; the stack is never
// collapsed into one affine map.
//
// Reverse mode.  With G_l the gradient at layer l's output,
//   grad t_l = sum_rows G_l,  grad s_l = sum_rows G_l z_{l-1} e_l + gld,
//   G_{l-1} = G_l e_l (+ gz_all[l-1]),  dx = G_0 e_0.
// A layer's input z_{l-1} is never rebuilt by inverting the layer (a
// contracting layer loses it): up to kRegL layers the forward sweep keeps every
// layer's input in registers; deeper stacks keep the input of every kSeg-th
// layer in registers and run the row forward from the nearest such checkpoint,
// at most kSeg - 1 steps.  There is no tape in the workspace.  The 2 D row sums
// per layer ([s | t], the flat gradient's own layout) live in per-lane
// accumulators when one lane holds a row of at most kAccD columns and
// L <= kRegL; otherwise each pass ends in a wave sum per word that one fixed lane adds into
// the wave's record (LDS, or the workspace when 4 records exceed 48 KB).  k_affine_finish adds the records in index order and adds the
// log-det's gradient to every s.  No float atomics, no inter-block dependency,
// no allocation, no host sync; every barrier sits under block-uniform bounds.
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

constexpr int kMaxL = CNF_AFFINE_MAX_LAYERS;
constexpr int kAccD = 10;  // per-lane accumulators up to this width
constexpr int kSeg = 16;   // deep stacks: a register checkpoint every kSeg layers
constexpr int kNSeg = (kMaxL + kSeg - 1) / kSeg;

struct Ptrs {
  const float* p[2 * kMaxL];
};

// per layer: the constant record [e | t | 8 scalars], 2 D row sums, no tape
Geo affine_geometry(int D, int L) { return geometry(D, L, 2 * padded_dim(D) + 8, 2 * D, 0); }
// reverse mode: every layer's input in registers up to kRegL layers; per-lane
// accumulators on top of it for one-lane rows of at most kAccD columns
constexpr BwdVariant affine_bwd_variant(int lpr, int cpl, int L) {
  const bool regt = L <= kRegL;
  return {regt, regt && lpr == 1 && cpl <= kAccD};
}
constexpr RowFamily kFamily{kMaxL, affine_geometry, affine_bwd_variant, 2};

// ---- per-layer constants --------------------------------------------------

__global__ __launch_bounds__(kThreads) void k_affine_prep(Ptrs P, float* __restrict__ blob, int D,
                                                          int dp, int cs, int L, int inv) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int k = wave; k < L; k += kWaves) {  // wave-uniform
    const int l = inv ? L - 1 - k : k;
    const float* __restrict__ s = P.p[2 * l];
    const float* __restrict__ sh = P.p[2 * l + 1];
    float* o = blob + (size_t)k * cs;
    float acc = 0.f;
    for (int j = lane; j < dp; j += 64) {
      float sv = j < D ? s[j] : 0.f;
      if (inv) sv = -sv;
      o[j] = j < D ? expf(sv) : 0.f;
      o[dp + j] = j < D ? sh[j] : 0.f;
      acc += sv;
    }
    acc = row_sum<64>(acc);
    if (lane < 8) o[2 * dp + lane] = lane == 0 ? acc : 0.f;
  }
  __syncthreads();
  if (t == 0) {
    float tot = 0.f;
    for (int k = 0; k < L; ++k) tot += blob[(size_t)k * cs + 2 * dp];
    blob[2 * dp + 1] = tot;
  }
}

// ---- row steps --------------------------------------------------------------

// One step on the row's registers, rounded as torch rounds it: no fused
// multiply-add.
template <int LPR, int CPL>
__device__ __forceinline__ void affine_step(float* xv, const float* __restrict__ cb, int gl,
                                            bool inv) {
  constexpr int DP = LPR * CPL;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const float e = cb[gl + LPR * k], t = cb[DP + gl + LPR * k];
    xv[k] = inv ? __fmul_rn(__fsub_rn(xv[k], t), e) : __fadd_rn(__fmul_rn(xv[k], e), t);
  }
}

__device__ __forceinline__ float ce_term(int kind, float lpy, bool yok) {
  const float ce = kind == CNF_LOSS_CAL ? -logf(expf(lpy) + 1e-7f) : -lpy;
  return yok ? ce : NAN;
}

// ---- forward / inverse ------------------------------------------------------

template <int LPR, int CPL>
__global__ __launch_bounds__(kThreads) void k_affine_fwd(
    const float* __restrict__ x, const float* __restrict__ blob, int D, int L, int cs, int64_t B,
    float* __restrict__ z, float* __restrict__ z_all, float* __restrict__ logdet,
    const int64_t* __restrict__ y, int kind, float ldw, float* __restrict__ part, int inv) {
  constexpr int RPB = kThreads / LPR;
  constexpr int DP = LPR * CPL;
  // one lane per row: the block's rows go through an LDS tile (odd row stride)
  // as coalesced sweeps; every loop bound below is block-uniform
  constexpr bool kStage = LPR == 1;
  constexpr int TS = CPL | 1;
  __shared__ float tile[kStage ? kThreads * TS : 1];
  __shared__ float red[kWaves * 2];
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR;
  const float ld = blob[2 * DP + 1];
  if (logdet && blockIdx.x == 0 && tid == 0) logdet[0] = ld;
  float t0 = 0.f, n0 = 0.f;
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
      affine_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, inv);
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
      const float ce = ce_term(kind, lpy, yy >= 0 && yy < D);
      if (valid && gl == 0) {
        t0 += ce;
        n0 += 1.f;
      }
    }
  }
  if (part) {  // block-uniform
    t0 = wave_sum_dpp63(t0);
    n0 = wave_sum_dpp63(n0);
    if ((tid & 63) == 63) {
      red[2 * (tid >> 6)] = t0;
      red[2 * (tid >> 6) + 1] = n0;
    }
    __syncthreads();
    if (tid == 0) {
      float s = 0.f, n = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        s += red[2 * w];
        n += red[2 * w + 1];
      }
      // (loss, ce, log-det, pad): the row's loss is ce - ldw * ld, ld the same for every row
      float* o = part + (size_t)blockIdx.x * 4;
      o[0] = s - ldw * (n * ld);
      o[1] = s;
      o[2] = n * ld;
      o[3] = 0.f;
    }
  }
}

// ---- predict ------------------------------------------------------------------

// Calibrator.predict of an affine flow calibrator (calibrators.py:40-44,
// 330-353), the row in registers from load to store: centre on the mean of the
// D real columns, run the stack, p = softmax(z), then
// softmax(log(p + 1e-7) - log_priors).  Padding columns hold 0 through the
// stack and enter no mean, maximum or sum.  Same grid, tile and barriers as
// k_affine_fwd.  SCORE: the scoring epilogue of cnf_score.h takes the fp32
// probabilities in place of the store phase.
template <int LPR, int CPL, bool SCORE>
__global__ __launch_bounds__(kThreads) void k_affine_predict(
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
    for (int l = 0; l < L; ++l) affine_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, false);
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
  int64_t B;
  int D, L, cs, ps, pw, gacc, kind;
  float ldw, gscale;    // the loss is ce - ldw * ld
};

// Backward through layer l.  In: zin = the layer's input, g = gradient at its
// output.  Out: g = gradient at its input; con[] = this row's 2 CPL
// contributions [grad s | grad t].  A row past the batch contributes exact
// zeros.
template <int LPR, int CPL>
__device__ __forceinline__ void affine_back(const float* zin, float* g, bool valid,
                                            const float* __restrict__ cb, int gl, float* con) {
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const float e = cb[gl + LPR * k];
    const float ge = g[k] * e;
    con[k] = valid ? ge * zin[k] : 0.f;
    con[CPL + k] = valid ? g[k] : 0.f;
    g[k] = valid ? ge : 0.f;
  }
}

// Add one row pass's contributions of layer l into the wave's record: a wave
// sum per word, added by one fixed lane (so the order is fixed).
template <int LPR, int CPL>
__device__ __forceinline__ void record_add(float* rec, const float* con, int gl, int lane, int D) {
  if constexpr (LPR == 1) {  // D == CPL
#pragma unroll
    for (int i = 0; i < 2 * CPL; ++i) {
      const float v = wave_sum_dpp63(con[i]);
      if (lane == 63) rec[i] += v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float a = col_sum<LPR>(con[k]);
      const float b = col_sum<LPR>(con[CPL + k]);
      const int c = gl + LPR * k;
      if (lane < LPR && c < D) {
        rec[c] += a;
        rec[D + c] += b;
      }
    }
  }
}

// The constant records come as a kernel argument of their own: a __restrict__
// argument is what lets the compiler read the per-layer constants of a
// one-lane row (a wave-uniform address) with scalar loads into SGPRs.  Read
// through the pointer in BwdArgs they were vector loads, 30 per layer and each
// waited on, with one wave per SIMD to hide nothing behind.
template <int LPR, int CPL, bool REGT, bool REGA>
__global__ __launch_bounds__(kThreads) void k_affine_bwd(BwdArgs A,
                                                         const float* __restrict__ blob) {
  constexpr int RL = kRegL;
  constexpr int RPB = kThreads / LPR;
  constexpr int DP = LPR * CPL;
  constexpr int NW = 2 * CPL;
  extern __shared__ float sm[];
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR, lane = tid & 63, wave = tid >> 6;
  const int D = A.D, L = A.L, cs = A.cs, ps = A.ps, pw = A.pw;
  const int64_t B = A.B;
  float* rec;  // this wave's record
  if (!A.gacc) {
    for (int i = tid; i < kWaves * pw; i += kThreads) sm[i] = 0.f;
    __syncthreads();
    rec = sm + wave * pw;
  } else {
    rec = A.part + ((size_t)blockIdx.x * kWaves + wave) * pw;  // zeroed by the host side
  }
  float racc[REGA ? RL * NW : 1];
#pragma unroll
  for (int i = 0; i < (REGA ? RL * NW : 1); ++i) racc[i] = 0.f;
  float t0 = 0.f, n0 = 0.f;

  for (int64_t base = (int64_t)blockIdx.x * RPB; base < B; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + gi;
    const bool valid = row < B;
    float xv[CPL], g[CPL], con[NW];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = gl + LPR * k;
      xv[k] = (valid && c < D) ? A.x[row * D + c] : 0.f;
    }
    // forward sweep: every layer's input (REGT) or every kSeg-th (checkpoints)
    float zt[REGT ? RL : kNSeg][CPL];
    if constexpr (REGT) {
#pragma unroll
      for (int l = 0; l < RL; ++l) {
        if (l < L) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) zt[l][k] = xv[k];
          affine_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, false);
        }
      }
    } else {
#pragma unroll
      for (int sg = 0; sg < kNSeg; ++sg) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) zt[sg][k] = xv[k];
        const int hi = (sg + 1) * kSeg < L ? (sg + 1) * kSeg : L;
        for (int l = sg * kSeg; l < hi; ++l)
          affine_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, false);
      }
    }
    // seed
    if (A.y) {
      const int64_t yy = valid ? A.y[row] : 0;
      const bool yok = yy >= 0 && yy < D;
      float m, lse, lpy;
      row_softmax<LPR, CPL>(xv, gl, D, yy, m, lse, lpy);
      const float ce = ce_term(A.kind, lpy, yok);
      if (valid && gl == 0) {
        t0 += ce;
        n0 += 1.f;
      }
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
      for (int l = RL - 1; l >= 0; --l) {
        if (l < L) {
          affine_back<LPR, CPL>(zt[l], g, valid, blob + (size_t)l * cs, gl, con);
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
#pragma unroll
      for (int sg = kNSeg - 1; sg >= 0; --sg) {
        const int hi = (sg + 1) * kSeg < L ? (sg + 1) * kSeg : L;
        for (int l = hi - 1; l >= sg * kSeg; --l) {  // block-uniform bounds
#pragma unroll
          for (int k = 0; k < CPL; ++k) xv[k] = zt[sg][k];
          for (int j = sg * kSeg; j < l; ++j)
            affine_step<LPR, CPL>(xv, blob + (size_t)j * cs, gl, false);
          affine_back<LPR, CPL>(xv, g, valid, blob + (size_t)l * cs, gl, con);
          record_add<LPR, CPL>(rec + l * ps, con, gl, lane, D);
          if (l > 0 && A.gz_all && valid) {
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
              const int c = gl + LPR * k;
              if (c < D) g[k] += A.gz_all[((int64_t)(l - 1) * B + row) * D + c];
            }
          }
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
    for (int l = 0; l < RL; ++l) {
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const float v = wave_sum_dpp63(racc[l * NW + i]);
        if (lane == 63 && l < L) rec[l * NW + i] = v;
      }
    }
  }
  t0 = wave_sum_dpp63(t0);
  n0 = wave_sum_dpp63(n0);
  if (lane == 63) {
    const float ld = blob[2 * DP + 1];
    rec[L * ps] = t0 - A.ldw * (n0 * ld);  // loss
    rec[L * ps + 1] = t0;                  // ce
    rec[L * ps + 2] = n0 * ld;             // log-det
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
// writes the three loss terms, then writes the flat gradient (s, t per layer:
// the record's own layout) with the log-det's gradient -- *gld when given,
// else gldv -- added to every s.
__global__ __launch_bounds__(kFinThreads) void k_affine_finish(
    const float* __restrict__ part, int units, int pw, int nsum, float* __restrict__ sums,
    float* __restrict__ terms, float* __restrict__ grads, const float* __restrict__ gld,
    float gldv, int D, int L) {
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
  const float gl = gld ? gld[0] : gldv;
  const int ps = 2 * D;
  for (int i = t; i < L * ps; i += kFinThreads) {
    const int j = i % ps;
    grads[i] = j < D ? sums[i] + gl : sums[i];
  }
}

// ---- launches -------------------------------------------------------------------

// the loss's weight of the log-det
float ld_weight(int32_t kind, float det) { return kind == CNF_LOSS_CAL ? 1.f : det; }

// What cnf_rowflow.h's launch layer asks of a family.
struct Affine {
  using Table = Ptrs;
  using Args = BwdArgs;
  static constexpr bool kLdScalar = true;  // the log-det is one number: [1]
  static const RowFamily& family() { return kFamily; }
  static constexpr int grad_floats(int D, int = 0) { return 2 * D; }  // s, t
  static int8_t* kinds(Ptrs&) { return nullptr; }

  static void prep(const Ptrs& P, const Geo& g, int D, int L, float* blob, bool inv,
                   hipStream_t s) {
    hipLaunchKernelGGL(k_affine_prep, dim3(1), dim3(kThreads), 0, s, P, blob, D, g.dp, g.cs, L,
                       inv ? 1 : 0);
  }

  template <int LPR, int CPL>
  static void fwd(int blocks, const FwdCall& c, const Geo& g, const float* blob, float* part) {
    hipLaunchKernelGGL((k_affine_fwd<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x, blob,
                       c.D, c.L, g.cs, c.B, c.z, c.z_all, c.ld, c.y, c.kind,
                       ld_weight(c.kind, c.det), part, c.inv ? 1 : 0);
  }

  template <int LPR, int CPL>
  static void predict(int blocks, const PredictCall& c, const Geo& g, const float* blob,
                      const score::Args* sc) {
    if (sc) {
      hipLaunchKernelGGL((k_affine_predict<LPR, CPL, true>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, (float*)nullptr, *sc);
    } else {
      hipLaunchKernelGGL((k_affine_predict<LPR, CPL, false>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, c.probs, score::Args{});
    }
  }

  template <int LPR, int CPL>
  static void bwd(int blocks, size_t lds, hipStream_t s, const BwdArgs& a) {
    if (!affine_bwd_variant(LPR, CPL, a.L).regt) {
      hipLaunchKernelGGL((k_affine_bwd<LPR, CPL, false, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a, a.blob);
      return;
    }
    // rega depends on the depth through regt alone: the geometry's answer at kRegL
    if constexpr (affine_bwd_variant(LPR, CPL, kRegL).rega) {
      hipLaunchKernelGGL((k_affine_bwd<LPR, CPL, true, true>), dim3(blocks), dim3(kThreads), lds,
                         s, a, a.blob);
    } else {
      hipLaunchKernelGGL((k_affine_bwd<LPR, CPL, true, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a, a.blob);
    }
  }

  static void fill(BwdArgs& a, const BwdCall& c, float*) { a.ldw = ld_weight(c.kind, c.det); }

  // c: the reverse call whose gradients this writes, null after a forward
  static void finish(const Finish& f, const Ptrs&, int D, int L, const Geo&, const BwdCall* c,
                     hipStream_t s) {
    // every row's loss holds -ldw * ld: the log-det's gradient is the rows' sum of it
    const bool loss = c && c->loss;
    const float ldw = loss ? ld_weight(c->kind, c->det) : 0.f;
    const float gldv = loss ? (float)(-(double)ldw * (double)c->gscale * (double)c->B) : 0.f;
    const float* gld = c && !loss ? c->gld : nullptr;
    hipLaunchKernelGGL(k_affine_finish, dim3(1), dim3(kFinThreads), 0, s, f.part, f.units, f.pw,
                       f.nsum, f.sums, f.terms, f.grads, gld, gldv, D, L);
  }
};

}  // namespace
}  // namespace cnf

extern "C" int cnf_affine_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats) {
  return cnf::rowflow::param_count(cnf::kFamily, cnf::Affine::grad_floats, dim, n_layers, n_floats);
}

extern "C" int cnf_affine_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B,
                                          size_t* bytes) {
  return cnf::rowflow::workspace_bytes(cnf::kFamily, dim, n_layers, B, bytes);
}

extern "C" int cnf_affine_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]) {
  return cnf::rowflow::launch_plan(cnf::kFamily, dim, n_layers, B, out);
}

extern "C" int cnf_affine_forward(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, float* z, float* logdet, float* z_all, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_affine_forward");
  return cnf::rowflow::run_forward<cnf::Affine>({dim, n_layers, params, x, nullptr, 0, 0.f, z,
                                                 logdet, z_all, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false,
                                                 false});
}

extern "C" int cnf_affine_inverse(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* z, float* x, float* logdet, float* x_all, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_affine_inverse");
  return cnf::rowflow::run_forward<cnf::Affine>({dim, n_layers, params, z, nullptr, 0, 0.f, x,
                                                 logdet, x_all, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false,
                                                 true});
}

extern "C" int cnf_affine_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                                       const float* x, const int64_t* y, int32_t loss_kind,
                                       float det, float* z, float* logdet, float* loss_terms,
                                       int64_t B, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  CNF_RANGE("cnf_affine_forward_loss");
  return cnf::rowflow::run_forward<cnf::Affine>({dim, n_layers, params, x, y, loss_kind, det, z,
                                                 logdet, nullptr, loss_terms, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true,
                                                 false});
}

extern "C" int cnf_affine_predict(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, const float* log_priors, float* probs, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_affine_predict");
  return cnf::rowflow::run_predict<cnf::Affine>({dim, n_layers, params, x, log_priors, probs,
                                                 nullptr, nullptr, 0, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false});
}

extern "C" int cnf_affine_score(int32_t dim, int32_t n_layers, const float* const* params,
                                const float* x, const float* log_priors, const int64_t* y,
                                int32_t bins, int64_t* record, int64_t B, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_affine_score");
  return cnf::rowflow::run_predict<cnf::Affine>({dim, n_layers, params, x, log_priors, nullptr,
                                                 nullptr, y, bins, record, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true});
}

extern "C" int cnf_affine_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                              const float* x, const float* gz, const float* gz_all,
                              const float* gld, float* grads, float* dx, int64_t B,
                              void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_affine_vjp");
  return cnf::rowflow::run_backward<cnf::Affine>({dim, n_layers, params, x, nullptr, 0, 0.f, 1.f,
                                                  gz, gz_all, gld, nullptr, grads, dx, B, workspace,
                                                  workspace_bytes, (hipStream_t)stream, false});
}

extern "C" int cnf_affine_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                                   const float* x, const int64_t* y, int32_t loss_kind, float det,
                                   float grad_scale, float* loss_terms, float* grads, float* dx,
                                   int64_t B, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  CNF_RANGE("cnf_affine_loss_vjp");
  return cnf::rowflow::run_backward<cnf::Affine>({dim, n_layers, params, x, y, loss_kind, det,
                                                  grad_scale, nullptr, nullptr, nullptr, loss_terms,
                                                  grads, dx, B, workspace, workspace_bytes,
                                                  (hipStream_t)stream, true});
}
