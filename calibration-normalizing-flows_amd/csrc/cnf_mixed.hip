// Mixed row-wise flows: a Flow whose layers are PlanarLayers, RadialLayers and
// AffineConstantLayers (both parameters) of one width, in any order, as fused
// HIP kernels: forward + per-row log-det (+ loss terms), the hand-derived
// reverse mode (+ fused loss seed), and the calibrator's predict with its
// score variant (cnf_score.h), all fp32.
//
// Geometry, grid caps, workspace plan, shape dispatch, the lane helpers and
// the host layer between the entry points and the launches (run_forward,
// run_predict, run_backward over this file's `Mixed` policy) are
// cnf_rowflow.h's, shared with cnf_planar.hip, cnf_radial.hip and
// cnf_affine.hip; the kernel bodies are this file's own text, as theirs are
// (DESIGN.md 7h).  What a mixed call has of its own -- `kinds`, checked
// directly after the shape, a parameter table packed 3 or 2 entries per layer
// and a gradient that is the per-kind sum -- the frame takes from
// RowFamily::kind_tensors and Mixed::grad_floats(D, kind).
//
// Per-layer constants.  k_mixed_prep (L blocks) writes one record of
// 2 DP + 8 floats per layer, whatever its kind (DP = LPR * CPL):
//   planar  [w[DP]  | u_hat[DP] | b, c = w.u_hat, wtu, m, ||w||, 0, 0, kind]
//   radial  [z0[DP] | 0[DP]     | a, sp, beta, sigmoid(b), 0, 0, 0, kind]
//   affine  [e[DP]  | t[DP]     | ld = sum_d s, 0, 0, 0, 0, 0, 0, kind]
// each computed as its family's prep kernel computes it.  The row kernels read
// that record and branch on the kind, which is the same for every lane of the
// grid: the branch is scalar.
//
// A layer is applied exactly as its family applies it (planar_step,
// radial_step, affine_step of the siblings); the stack is never collapsed.  The
// log-det is a row's: 0, then one rounded fp32 addition per planar layer (the
// row's term) and per affine layer (ld), in layer order.
//
// Reverse mode.  No layer is ever inverted: an affine layer that contracts
// loses its input, and a chain of radial inversions grows the rebuilt row's
// error.  Up to kRegL layers the forward sweep keeps every layer's input in
// registers; deeper stacks keep the input of every kSeg-th layer in registers
// and run the row forward again from the nearest such checkpoint, at most
// kSeg - 1 steps.  Both arrays are indexed by unrolled loops only.  There is
// no tape in the workspace.  From a layer's input the backward step recomputes
// what it needs (planar: h = tanh(x.w + b); radial: d, r, h).  The row sums
// per layer are one uniform 2 D + 2 words:
//   planar  [h g [D] | g_a x [D] | G_c, G_b]
//   radial  [g_d [D] | 0 [D]     | h s, g_r]
//   affine  [g e x [D] | g [D]   | sum gld, 0]
// in per-lane accumulators when one lane holds a row of at most kAccD columns
// and L <= kRegL (wider one-lane rows take the checkpointed kernel at every
// depth); otherwise each pass ends in a wave sum per word that one
// fixed lane adds into the wave's record (LDS, or the workspace when 4 records
// exceed 48 KB).  k_mixed_finish adds the records in index order, applies each
// layer's chain rule by kind and writes the flat gradient at the layer's
// offset.  No float atomics, no inter-block dependency, no allocation, no host
// sync; every barrier sits under block-uniform bounds.
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

constexpr int kMaxL = CNF_MIXED_MAX_LAYERS;
constexpr int kAccD = 10;  // per-lane accumulators up to this width
constexpr int kSeg = 16;   // deep stacks: a register checkpoint every kSeg layers
constexpr int kNSeg = (kMaxL + kSeg - 1) / kSeg;

// Three slots per layer on the device side (an affine layer's third is null);
// the caller's table is packed, 3 or 2 entries per layer.
struct Ptrs {
  const float* p[3 * kMaxL];
};
struct Kinds {
  int8_t k[kMaxL];
};

// per layer: the constant record [DP | DP | 8 scalars], 2 D + 2 row sums, no tape
Geo mixed_geometry(int D, int L) { return geometry(D, L, 2 * padded_dim(D) + 8, 2 * D + 2, 0); }
// reverse mode: every layer's input in registers up to kRegL layers, with
// per-lane accumulators for a one-lane row.  A one-lane row wider than kAccD
// columns has no room for the accumulators, and built without them (2 D + 2
// wave sums per layer and kind in the unrolled sweep) its input array went to
// scratch: those widths take the checkpointed kernel at every
// depth.
constexpr BwdVariant mixed_bwd_variant(int lpr, int cpl, int L) {
  const bool regt = L <= kRegL && (lpr != 1 || cpl <= kAccD);
  return {regt, regt && lpr == 1};
}

constexpr int tensors_of(int kind) { return kind == CNF_LAYER_AFFINE ? 2 : 3; }
// gradient (= parameter) floats of a layer: w, u, b / z0, a, b / s, t
__host__ __device__ constexpr int grad_floats(int kind, int D) {
  return kind == CNF_LAYER_PLANAR ? 2 * D + 1 : kind == CNF_LAYER_RADIAL ? D + 2 : 2 * D;
}

// ---- per-layer constants --------------------------------------------------

__global__ __launch_bounds__(64) void k_mixed_prep(Ptrs P, Kinds K, float* __restrict__ blob, int D,
                                                   int dp, int cs) {
  const int l = blockIdx.x, t = threadIdx.x;
  const int kd = K.k[l];  // block-uniform
  float* o = blob + (size_t)l * cs;
  if (kd == CNF_LAYER_PLANAR) {
    const float* w = P.p[3 * l];
    const float* u = P.p[3 * l + 1];
    const float* b = P.p[3 * l + 2];
    // the one evaluation of the reference's scalars (flows/flows.py:150-153)
    float wtu = 0.f, n2 = 0.f;
    for (int j = 0; j < D; ++j) {
      wtu = fmaf(w[j], u[j], wtu);
      n2 = fmaf(w[j], w[j], n2);
    }
    const float m = -1.f + log1pf(expf(wtu));
    const float nrm = sqrtf(n2);
    for (int j = t; j < dp; j += 64) {
      o[j] = j < D ? w[j] : 0.f;
      // u + ((m - wtu) * w) / ||w||, the reference's order; ||w|| = 0 gives NaN
      float uh = 0.f;
      if (j < D) {
        const float num = (m - wtu) * w[j];
        uh = u[j] + num / nrm;
      }
      o[dp + j] = uh;
    }
    __syncthreads();
    if (t == 0) {
      float c = 0.f;
      for (int j = 0; j < D; ++j) c = fmaf(o[j], o[dp + j], c);
      o[2 * dp] = b[0];
      o[2 * dp + 1] = c;
      o[2 * dp + 2] = wtu;
      o[2 * dp + 3] = m;
      o[2 * dp + 4] = nrm;
      o[2 * dp + 5] = 0.f;
      o[2 * dp + 6] = 0.f;
      o[2 * dp + 7] = (float)kd;
    }
  } else if (kd == CNF_LAYER_RADIAL) {
    const float* z0 = P.p[3 * l];
    for (int j = t; j < dp; j += 64) {
      o[j] = j < D ? z0[j] : 0.f;
      o[dp + j] = 0.f;
    }
    if (t == 0) {
      const float a = P.p[3 * l + 1][0];
      const float b = P.p[3 * l + 2][0];
      const float sp = log1pf(expf(b));
      o[2 * dp] = a;
      o[2 * dp + 1] = sp;
      o[2 * dp + 2] = -a + sp;
      o[2 * dp + 3] = 1.f / (1.f + expf(-b));
      o[2 * dp + 4] = 0.f;
      o[2 * dp + 5] = 0.f;
      o[2 * dp + 6] = 0.f;
      o[2 * dp + 7] = (float)kd;
    }
  } else {
    const float* s = P.p[3 * l];
    const float* sh = P.p[3 * l + 1];
    float acc = 0.f;
    for (int j = t; j < dp; j += 64) {
      const float sv = j < D ? s[j] : 0.f;
      o[j] = j < D ? expf(sv) : 0.f;
      o[dp + j] = j < D ? sh[j] : 0.f;
      acc += sv;
    }
    acc = row_sum<64>(acc);
    if (t < 8) o[2 * dp + t] = t == 0 ? acc : t == 7 ? (float)kd : 0.f;
  }
}

// ---- row steps --------------------------------------------------------------

// the kind of the layer whose record is cb: the same for every lane of the grid
template <int DP>
__device__ __forceinline__ int layer_kind(const float* __restrict__ cb) {
  return (int)cb[2 * DP + 7];
}

// One layer forward on the row's registers, by kind; adds the layer's log-det
// to the row's.  Padding columns hold 0 in xv and in every vector of the
// record, so they stay 0 and add nothing to a dot product or a norm.
template <int LPR, int CPL>
__device__ __forceinline__ void mixed_step(float* xv, const float* __restrict__ cb, int gl,
                                           float& ld) {
  constexpr int DP = LPR * CPL;
  const int kd = layer_kind<DP>(cb);
  if (kd == CNF_LAYER_PLANAR) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) a = fmaf(xv[k], cb[gl + LPR * k], a);
    a = row_sum<LPR>(a) + cb[2 * DP];
    const float h = tanhf(a);
#pragma unroll
    for (int k = 0; k < CPL; ++k) xv[k] = fmaf(h, cb[DP + gl + LPR * k], xv[k]);
    ld += logf(fabsf(1.f + (1.f - h * h) * cb[2 * DP + 1]));
  } else if (kd == CNF_LAYER_RADIAL) {
    float d[CPL];
    float r2 = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      d[k] = xv[k] - cb[gl + LPR * k];
      r2 = fmaf(d[k], d[k], r2);
    }
    const float r = sqrtf(row_sum<LPR>(r2));
    const float h = 1.f / (cb[2 * DP] + r);
    const float bh = cb[2 * DP + 2] * h;
#pragma unroll
    for (int k = 0; k < CPL; ++k) xv[k] = fmaf(bh, d[k], xv[k]);
  } else {
    // rounded as torch rounds it: a product, then a sum
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      xv[k] = __fadd_rn(__fmul_rn(xv[k], cb[gl + LPR * k]), cb[DP + gl + LPR * k]);
    ld = __fadd_rn(ld, cb[2 * DP]);
  }
}

__device__ __forceinline__ void loss_terms(int kind, float det, float lpy, float ld, bool yok,
                                           float& loss, float& ce) {
  if (kind == CNF_LOSS_CAL) {
    ce = -logf(expf(lpy) + 1e-7f);
    loss = ce - ld;
  } else {
    ce = -lpy;
    loss = ce - det * ld;
  }
  if (!yok) ce = loss = NAN;
}

// ---- forward ----------------------------------------------------------------

template <int LPR, int CPL>
__global__ __launch_bounds__(kThreads) void k_mixed_fwd(
    const float* __restrict__ x, const float* __restrict__ blob, int D, int L, int cs, int64_t B,
    float* __restrict__ z, float* __restrict__ ld_out, float* __restrict__ z_all,
    const int64_t* __restrict__ y, int kind, float det, float* __restrict__ part) {
  constexpr int RPB = kThreads / LPR;
  // one lane per row (D == CPL): the block's rows go through an LDS tile (odd
  // row stride) as coalesced sweeps; every loop bound below is block-uniform
  constexpr bool kStage = LPR == 1;
  constexpr int TS = CPL | 1;
  __shared__ float tile[kStage ? kThreads * TS : 1];
  __shared__ float red[kWaves * 4];
  const int tid = threadIdx.x, gl = tid % LPR, gi = tid / LPR;
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
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
    float ld = 0.f;
    for (int l = 0; l < L; ++l) {
      mixed_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
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
    if (valid && ld_out && gl == 0) ld_out[row] = ld;
    if (y) {
      const int64_t yy = valid ? y[row] : 0;
      float m, lse, lpy, loss, ce;
      row_softmax<LPR, CPL>(xv, gl, D, yy, m, lse, lpy);
      loss_terms(kind, det, lpy, ld, yy >= 0 && yy < D, loss, ce);
      if (valid && gl == 0) {
        t0 += loss;
        t1 += ce;
        t2 += ld;
      }
    }
  }
  if (part) {  // block-uniform
    t0 = wave_sum_dpp63(t0);
    t1 = wave_sum_dpp63(t1);
    t2 = wave_sum_dpp63(t2);
    if ((tid & 63) == 63) {
      red[4 * (tid >> 6)] = t0;
      red[4 * (tid >> 6) + 1] = t1;
      red[4 * (tid >> 6) + 2] = t2;
      red[4 * (tid >> 6) + 3] = 0.f;
    }
    __syncthreads();
    if (tid < 4) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += red[4 * w + tid];
      part[(size_t)blockIdx.x * 4 + tid] = s;
    }
  }
}

// ---- predict ------------------------------------------------------------------

// Calibrator.predict of a mixed flow calibrator (calibrators.py:40-44,
// 330-353), the row in registers from load to store: centre on the mean of the
// D real columns, run the stack, p = softmax(z), then
// softmax(log(p + 1e-7) - log_priors).  Padding columns hold 0 through the
// stack and enter no mean, norm, maximum or sum.  Same grid, tile and barriers
// as k_mixed_fwd.  SCORE: the scoring epilogue of cnf_score.h takes the fp32
// probabilities in place of the store phase, and the log-det is not written.
template <int LPR, int CPL, bool SCORE>
__global__ __launch_bounds__(kThreads) void k_mixed_predict(
    const float* __restrict__ x, const float* __restrict__ blob, const float* __restrict__ lp,
    int D, int L, int cs, int64_t B, float* __restrict__ probs, float* __restrict__ ld_out,
    score::Args sc) {
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
    float ld = 0.f;
    for (int l = 0; l < L; ++l) mixed_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
    if constexpr (!SCORE) {
      if (valid && ld_out && gl == 0) ld_out[row] = ld;
    }
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
  const float* gld;     // [B]
  float* dx;
  float* part;          // block records (wave records when gacc)
  int64_t B;
  int D, L, cs, ps, pw, gacc, kind;
  float det, gscale;
};

// Backward through layer l, by kind.  In: zin = the layer's input, g =
// gradient at its output, gam = gradient at the row's log-det.  Out: g =
// gradient at its input; con[] = this row's 2 CPL + 2 contributions in the
// layout at the head of this file.  A row past the batch contributes exact
// zeros and keeps g at 0.
template <int LPR, int CPL>
__device__ __forceinline__ void mixed_back(const float* zin, float* g, float gam, bool valid,
                                           const float* __restrict__ cb, int gl, float* con) {
  constexpr int DP = LPR * CPL;
  const int kd = layer_kind<DP>(cb);
  if (kd == CNF_LAYER_PLANAR) {
    float a = 0.f, s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      a = fmaf(zin[k], cb[gl + LPR * k], a);
      s = fmaf(g[k], cb[DP + gl + LPR * k], s);
    }
    a = row_sum<LPR>(a) + cb[2 * DP];
    s = row_sum<LPR>(s);
    const float h = tanhf(a);
    const float c = cb[2 * DP + 1];
    const float hp = 1.f - h * h;
    const float q = 1.f + hp * c;
    float ga = s * hp + gam * (c / q) * (-2.f * h * hp);
    float gc = gam * hp / q;
    if (!valid) ga = gc = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      con[k] = valid ? h * g[k] : 0.f;
      con[CPL + k] = valid ? ga * zin[k] : 0.f;
      g[k] = valid ? fmaf(ga, cb[gl + LPR * k], g[k]) : 0.f;
    }
    con[2 * CPL] = gc;
    con[2 * CPL + 1] = ga;
  } else if (kd == CNF_LAYER_RADIAL) {
    const float a = cb[2 * DP], beta = cb[2 * DP + 2];
    float d[CPL];
    float r2 = 0.f, s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      d[k] = zin[k] - cb[gl + LPR * k];
      r2 = fmaf(d[k], d[k], r2);
      s = fmaf(g[k], d[k], s);
    }
    const float r = sqrtf(row_sum<LPR>(r2));
    s = row_sum<LPR>(s);
    const float h = 1.f / (a + r);
    const float hs = h * s;
    const float gr = -h * beta * hs;
    const float gq = r != 0.f ? gr / r : 0.f;  // torch's norm backward: 0 at r == 0
    const float bh = beta * h;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float gd = fmaf(gq, d[k], bh * g[k]);
      con[k] = valid ? gd : 0.f;
      con[CPL + k] = 0.f;
      g[k] = valid ? g[k] + gd : 0.f;
    }
    con[2 * CPL] = valid ? hs : 0.f;
    con[2 * CPL + 1] = valid ? gr : 0.f;
  } else {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float ge = g[k] * cb[gl + LPR * k];
      con[k] = valid ? ge * zin[k] : 0.f;
      con[CPL + k] = valid ? g[k] : 0.f;
      g[k] = valid ? ge : 0.f;
    }
    con[2 * CPL] = valid ? gam : 0.f;  // every s of the layer takes the rows' sum of it
    con[2 * CPL + 1] = 0.f;
  }
}

// Add one row pass's contributions of layer l into the wave's record: a wave
// sum per word, added by one fixed lane (so the order is fixed).
template <int LPR, int CPL>
__device__ __forceinline__ void record_add(float* rec, const float* con, int gl, int lane, int D) {
  if constexpr (LPR == 1) {
#pragma unroll
    for (int i = 0; i < 2 * CPL + 2; ++i) {
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
    const float gc = col_sum<LPR>(con[2 * CPL]);
    const float gb = col_sum<LPR>(con[2 * CPL + 1]);
    if (lane == 0) {
      rec[2 * D] += gc;
      rec[2 * D + 1] += gb;
    }
  }
}

// The constant records come as a kernel argument of their own: a __restrict__
// argument lets the compiler read a one-lane row's per-layer constants (a
// wave-uniform address) with scalar loads.
template <int LPR, int CPL, bool REGT, bool REGA>
__global__ __launch_bounds__(kThreads) void k_mixed_bwd(BwdArgs A, const float* __restrict__ blob) {
  constexpr int RL = kRegL;
  constexpr int RPB = kThreads / LPR;
  constexpr int NW = 2 * CPL + 2;
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
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;

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
    float ld = 0.f;
    if constexpr (REGT) {
#pragma unroll
      for (int l = 0; l < RL; ++l) {
        if (l < L) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) zt[l][k] = xv[k];
          mixed_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
        }
      }
    } else {
#pragma unroll
      for (int sg = 0; sg < kNSeg; ++sg) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) zt[sg][k] = xv[k];
        const int hi = (sg + 1) * kSeg < L ? (sg + 1) * kSeg : L;
        for (int l = sg * kSeg; l < hi; ++l)
          mixed_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
      }
    }
    // seed
    float gam;
    if (A.y) {
      const int64_t yy = valid ? A.y[row] : 0;
      const bool yok = yy >= 0 && yy < D;
      float m, lse, lpy, loss, ce;
      row_softmax<LPR, CPL>(xv, gl, D, yy, m, lse, lpy);
      loss_terms(A.kind, A.det, lpy, ld, yok, loss, ce);
      if (valid && gl == 0) {
        t0 += loss;
        t1 += ce;
        t2 += ld;
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
      gam = valid ? -A.gscale * (A.kind == CNF_LOSS_CAL ? 1.f : A.det) : 0.f;
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
      gam = (valid && A.gld) ? A.gld[row] : 0.f;
    }
    // backward sweep
    if constexpr (REGT) {
#pragma unroll
      for (int l = RL - 1; l >= 0; --l) {
        if (l < L) {
          mixed_back<LPR, CPL>(zt[l], g, gam, valid, blob + (size_t)l * cs, gl, con);
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
          float skip = 0.f;
#pragma unroll
          for (int k = 0; k < CPL; ++k) xv[k] = zt[sg][k];
          for (int j = sg * kSeg; j < l; ++j)
            mixed_step<LPR, CPL>(xv, blob + (size_t)j * cs, gl, skip);
          mixed_back<LPR, CPL>(xv, g, gam, valid, blob + (size_t)l * cs, gl, con);
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
  t1 = wave_sum_dpp63(t1);
  t2 = wave_sum_dpp63(t2);
  if (lane == 63) {
    rec[L * ps] = t0;
    rec[L * ps + 1] = t1;
    rec[L * ps + 2] = t2;
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
// writes the three loss terms, then applies each layer's chain rule by kind --
// planar through u_hat, radial through beta = log1p(exp(b)) - a, affine adding
// the rows' sum of the log-det's gradient to every s -- and writes the flat
// gradient at the layer's offset.
__global__ __launch_bounds__(kFinThreads) void k_mixed_finish(
    const float* __restrict__ part, int units, int pw, int nsum, float* __restrict__ sums,
    float* __restrict__ terms, float* __restrict__ grads, const float* __restrict__ blob, Ptrs P,
    Kinds K, int D, int L, int dp, int cs) {
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
  if (t < L) {
    const int l = t, ps = 2 * D + 2;
    int off = 0;
    for (int j = 0; j < l; ++j) off += grad_floats(K.k[j], D);
    const int kd = K.k[l];
    const float* cb = blob + (size_t)l * cs;
    const float* S = sums + (size_t)l * ps;
    float* go = grads + off;
    if (kd == CNF_LAYER_PLANAR) {
      const float* u = P.p[3 * l + 1];
      const float wtu = cb[2 * dp + 2], m = cb[2 * dp + 3], nrm = cb[2 * dp + 4];
      const float gc = S[2 * D], gb = S[2 * D + 1];
      const float k = (m - wtu) / nrm;
      const float sig = 1.f / (1.f + expf(-wtu));
      float tt = 0.f;
      for (int j = 0; j < D; ++j) tt = fmaf(S[j] + gc * cb[j], cb[j], tt);
      const float gwtu = tt * (sig - 1.f) / nrm;
      const float tk = tt * k / (nrm * nrm);
      for (int j = 0; j < D; ++j) {
        const float w = cb[j];
        const float gu = S[j] + gc * w;
        const float gw = S[D + j] + gc * cb[dp + j];
        go[D + j] = gu + gwtu * w;
        go[j] = gw + k * gu + gwtu * u[j] - tk * w;
      }
      go[2 * D] = gb;
    } else if (kd == CNF_LAYER_RADIAL) {
      // dL/dz0 = -sum g_d,  dL/da = sum g_r - g_beta,  dL/db = g_beta sigmoid(b)
      for (int j = 0; j < D; ++j) go[j] = -S[j];
      go[D] = S[2 * D + 1] - S[2 * D];
      go[D + 1] = S[2 * D] * cb[2 * dp + 3];
    } else {
      const float gl = S[2 * D];
      for (int j = 0; j < D; ++j) {
        go[j] = S[j] + gl;
        go[D + j] = S[D + j];
      }
    }
  }
}

// ---- launches -------------------------------------------------------------------

constexpr RowFamily kFamily{kMaxL, mixed_geometry, mixed_bwd_variant, 3, tensors_of};

// What cnf_rowflow.h's launch layer asks of a family.
struct Mixed {
  // host only: the kernels take the two by value, separately
  struct Table : Ptrs {
    Kinds K;
  };
  using Args = BwdArgs;
  static constexpr bool kLdScalar = false;  // the log-det is a row's: [B]
  static const RowFamily& family() { return kFamily; }
  static constexpr int grad_floats(int D, int kind) { return cnf::grad_floats(kind, D); }
  static int8_t* kinds(Table& T) { return T.K.k; }

  static void prep(const Table& T, const Geo& g, int D, int L, float* blob, bool, hipStream_t s) {
    hipLaunchKernelGGL(k_mixed_prep, dim3(L), dim3(64), 0, s, (const Ptrs&)T, T.K, blob, D, g.dp,
                       g.cs);
  }

  template <int LPR, int CPL>
  static void fwd(int blocks, const FwdCall& c, const Geo& g, const float* blob, float* part) {
    hipLaunchKernelGGL((k_mixed_fwd<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x, blob,
                       c.D, c.L, g.cs, c.B, c.z, c.ld, c.z_all, c.y, c.kind, c.det, part);
  }

  template <int LPR, int CPL>
  static void predict(int blocks, const PredictCall& c, const Geo& g, const float* blob,
                      const score::Args* sc) {
    if (sc) {
      hipLaunchKernelGGL((k_mixed_predict<LPR, CPL, true>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, (float*)nullptr, (float*)nullptr,
                         *sc);
    } else {
      hipLaunchKernelGGL((k_mixed_predict<LPR, CPL, false>), dim3(blocks), dim3(kThreads), 0, c.s,
                         c.x, blob, c.lp, c.D, c.L, g.cs, c.B, c.probs, c.ld, score::Args{});
    }
  }

  template <int LPR, int CPL>
  static void bwd(int blocks, size_t lds, hipStream_t s, const BwdArgs& a) {
    if (!mixed_bwd_variant(LPR, CPL, a.L).regt) {
      hipLaunchKernelGGL((k_mixed_bwd<LPR, CPL, false, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a, a.blob);
      return;
    }
    // regt and rega depend on the depth through L <= kRegL alone: the geometry's
    // answer at kRegL
    if constexpr (!mixed_bwd_variant(LPR, CPL, kRegL).regt) {
      return;  // not reached: the branch above took every depth
    } else if constexpr (mixed_bwd_variant(LPR, CPL, kRegL).rega) {
      hipLaunchKernelGGL((k_mixed_bwd<LPR, CPL, true, true>), dim3(blocks), dim3(kThreads), lds, s,
                         a, a.blob);
    } else {
      hipLaunchKernelGGL((k_mixed_bwd<LPR, CPL, true, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a, a.blob);
    }
  }

  static void fill(BwdArgs& a, const BwdCall& c, float*) {  // no tape
    a.gld = c.loss ? nullptr : c.gld;
    a.det = c.det;
  }

  static void finish(const Finish& f, const Table& T, int D, int L, const Geo& g, const BwdCall*,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_mixed_finish, dim3(1), dim3(kFinThreads), 0, s, f.part, f.units, f.pw,
                       f.nsum, f.sums, f.terms, f.grads, f.blob, (const Ptrs&)T, T.K, D, L, g.dp,
                       g.cs);
  }
};

}  // namespace
}  // namespace cnf

extern "C" int cnf_mixed_param_count(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                     int64_t* n_floats) {
  return cnf::rowflow::param_count(cnf::kFamily, cnf::Mixed::grad_floats, dim, n_layers, n_floats,
                                   kinds);
}

extern "C" int cnf_mixed_workspace_bytes(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                         int64_t B, size_t* bytes) {
  return cnf::rowflow::workspace_bytes(cnf::kFamily, dim, n_layers, B, bytes, kinds);
}

extern "C" int cnf_mixed_launch_plan(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                     int64_t B, int32_t out[8]) {
  return cnf::rowflow::launch_plan(cnf::kFamily, dim, n_layers, B, out, kinds);
}

extern "C" int cnf_mixed_forward(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                 const float* const* params, const float* x, float* z,
                                 float* logdet, float* z_all, int64_t B, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_forward");
  return cnf::rowflow::run_forward<cnf::Mixed>({dim, n_layers, params, x, nullptr, 0, 0.f, z,
                                                logdet, z_all, nullptr, B, workspace,
                                                workspace_bytes, (hipStream_t)stream, false, false,
                                                kinds});
}

extern "C" int cnf_mixed_forward_loss(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                      const float* const* params, const float* x,
                                      const int64_t* y, int32_t loss_kind, float det, float* z,
                                      float* logdet, float* loss_terms, int64_t B, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_forward_loss");
  return cnf::rowflow::run_forward<cnf::Mixed>({dim, n_layers, params, x, y, loss_kind, det, z,
                                                logdet, nullptr, loss_terms, B, workspace,
                                                workspace_bytes, (hipStream_t)stream, true, false,
                                                kinds});
}

extern "C" int cnf_mixed_predict(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                 const float* const* params, const float* x,
                                 const float* log_priors, float* probs, float* logdet, int64_t B,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_predict");
  return cnf::rowflow::run_predict<cnf::Mixed>({dim, n_layers, params, x, log_priors, probs,
                                                logdet, nullptr, 0, nullptr, B, workspace,
                                                workspace_bytes, (hipStream_t)stream, false,
                                                kinds});
}

extern "C" int cnf_mixed_score(int32_t dim, int32_t n_layers, const int32_t* kinds,
                               const float* const* params, const float* x, const float* log_priors,
                               const int64_t* y, int32_t bins, int64_t* record, int64_t B,
                               void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_score");
  return cnf::rowflow::run_predict<cnf::Mixed>({dim, n_layers, params, x, log_priors, nullptr,
                                                nullptr, y, bins, record, B, workspace,
                                                workspace_bytes, (hipStream_t)stream, true, kinds});
}

extern "C" int cnf_mixed_vjp(int32_t dim, int32_t n_layers, const int32_t* kinds,
                             const float* const* params, const float* x, const float* gz,
                             const float* gz_all, const float* gld, float* grads, float* dx,
                             int64_t B, void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_vjp");
  return cnf::rowflow::run_backward<cnf::Mixed>({dim, n_layers, params, x, nullptr, 0, 0.f, 1.f,
                                                 gz, gz_all, gld, nullptr, grads, dx, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false,
                                                 kinds});
}

extern "C" int cnf_mixed_loss_vjp(int32_t dim, int32_t n_layers, const int32_t* kinds,
                                  const float* const* params, const float* x, const int64_t* y,
                                  int32_t loss_kind, float det, float grad_scale,
                                  float* loss_terms, float* grads, float* dx, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_mixed_loss_vjp");
  return cnf::rowflow::run_backward<cnf::Mixed>({dim, n_layers, params, x, y, loss_kind, det,
                                                 grad_scale, nullptr, nullptr, nullptr, loss_terms,
                                                 grads, dx, B, workspace, workspace_bytes,
                                                 (hipStream_t)stream, true, kinds});
}
