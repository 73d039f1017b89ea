// Planar flows (the reference's PlanarLayer, flows/flows.py:129-165) as fused
// HIP kernels: forward + log-det (+ loss terms), and the hand-derived reverse
// mode (+ fused loss seed), and the calibrator's predict (centring, the stack,
// both softmaxes and the prior correction in one pass) with its score variant
// (the predict ending in cnf_metrics' record, cnf_score.h), all fp32.
//
// Rows: one lane per row for D <= 16 (the row in registers), 16 lanes per row
// for D <= 64, 64 lanes per row above (column c of a row sits in lane c % LPR,
// slot c / LPR; dot products end in an xor butterfly over the row's lanes).
// Every kernel walks the batch in a grid-stride loop under a fixed grid cap,
// so the order of every sum depends on (D, L, B) only.  The forward kernel's
// one-lane rows move through an LDS tile as coalesced sweeps.
//
// Per-layer constants.  k_planar_prep (L blocks) writes, per layer,
//   [w[DP] | u_hat[DP] | b, c, wtu, m, ||w||, 0, 0, 0]      DP = LPR * CPL
// into the caller's workspace; the row kernels and the finish step read that
// one record, so forward, reverse and the chain rule see the same bits.
//
// Reverse mode.  The forward sweep keeps one h per (row, layer): in registers
// up to kRegL layers, in an [L][B] tape in the workspace above.  The backward
// sweep rebuilds x_l = z_l - h_l u_hat_l.  The 2D+2 row sums per layer live in
// per-lane accumulators over the whole grid-stride loop when D <= kAccD and
// L <= kRegL (one wave sum at the end); otherwise each pass ends in a wave sum
// per word that one fixed lane adds into the wave's record (LDS, or the
// workspace when 4 records exceed 48 KB).  Block (or wave) records go to the
// workspace; k_planar_finish adds them in index order, applies the per-layer
// chain rule through u_hat and writes the flat gradient (w, u, b per layer).
// No float atomics, no inter-block dependency, no allocation, no host sync.
//
// Geometry, grid caps, workspace plan, argument checks, shape dispatch and the
// lane helpers are cnf_rowflow.h's, shared with cnf_radial.hip; the kernel
// bodies are this file's own text.
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

constexpr int kMaxL = CNF_PLANAR_MAX_LAYERS;
constexpr int kAccD = 11;  // per-lane accumulators: kRegL * (2 * 11 + 2) = 240 floats

struct Ptrs {
  const float* p[3 * kMaxL];
};

// per layer: the constant record [w | u_hat | 8 scalars], 2 D + 2 row sums
Geo planar_geometry(int D, int L) { return geometry(D, L, 2 * padded_dim(D) + 8, 2 * D + 2); }
// reverse mode: the tape in registers up to kRegL layers; per-lane accumulators
// on top of it for one-lane rows of at most kAccD columns
constexpr BwdVariant planar_bwd_variant(int lpr, int cpl, int L) {
  const bool regt = L <= kRegL;
  return {regt, regt && lpr == 1 && cpl <= kAccD};
}
constexpr RowFamily kFamily{kMaxL, planar_geometry, planar_bwd_variant};

// ---- per-layer constants --------------------------------------------------

struct LayerScalars {
  float wtu, m, nrm;
};

// The one evaluation of the reference's scalars (flows/flows.py:150-153).
__device__ __forceinline__ LayerScalars planar_scalars(const float* __restrict__ w,
                                                       const float* __restrict__ u, int D) {
  float wtu = 0.f, n2 = 0.f;
  for (int j = 0; j < D; ++j) {
    wtu = fmaf(w[j], u[j], wtu);
    n2 = fmaf(w[j], w[j], n2);
  }
  LayerScalars s;
  s.wtu = wtu;
  s.m = -1.f + log1pf(expf(wtu));
  s.nrm = sqrtf(n2);
  return s;
}

// u + ((m - wtu) * w) / ||w||, the reference's order; ||w|| = 0 gives NaN
__device__ __forceinline__ float planar_uhat(const LayerScalars& s, float w, float u) {
  const float num = (s.m - s.wtu) * w;
  return u + num / s.nrm;
}

__global__ __launch_bounds__(64) void k_planar_prep(Ptrs P, float* __restrict__ blob, int D, int dp,
                                                    int cs) {
  const int l = blockIdx.x, t = threadIdx.x;
  const float* w = P.p[3 * l];
  const float* u = P.p[3 * l + 1];
  const float* b = P.p[3 * l + 2];
  float* o = blob + (size_t)l * cs;
  const LayerScalars s = planar_scalars(w, u, D);
  for (int j = t; j < dp; j += 64) {
    o[j] = j < D ? w[j] : 0.f;
    o[dp + j] = j < D ? planar_uhat(s, w[j], u[j]) : 0.f;
  }
  __syncthreads();
  if (t == 0) {
    float c = 0.f;
    for (int j = 0; j < D; ++j) c = fmaf(o[j], o[dp + j], c);
    o[2 * dp] = b[0];
    o[2 * dp + 1] = c;
    o[2 * dp + 2] = s.wtu;
    o[2 * dp + 3] = s.m;
    o[2 * dp + 4] = s.nrm;
    o[2 * dp + 5] = 0.f;
    o[2 * dp + 6] = 0.f;
    o[2 * dp + 7] = 0.f;
  }
}

// ---- row steps --------------------------------------------------------------

// One layer forward on the row's registers; returns h, adds the log-det.
template <int LPR, int CPL>
__device__ __forceinline__ float planar_step(float* xv, const float* __restrict__ cb, int gl,
                                             float& ld) {
  constexpr int DP = LPR * CPL;
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) a = fmaf(xv[k], cb[gl + LPR * k], a);
  a = row_sum<LPR>(a) + cb[2 * DP];
  const float h = tanhf(a);
#pragma unroll
  for (int k = 0; k < CPL; ++k) xv[k] = fmaf(h, cb[DP + gl + LPR * k], xv[k]);
  ld += logf(fabsf(1.f + (1.f - h * h) * cb[2 * DP + 1]));
  return h;
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
__global__ __launch_bounds__(kThreads) void k_planar_fwd(
    const float* __restrict__ x, const float* __restrict__ blob, int D, int L, int cs, int64_t B,
    float* __restrict__ z, float* __restrict__ ld_out, float* __restrict__ z_all,
    const int64_t* __restrict__ y, int kind, float det, float* __restrict__ part) {
  constexpr int RPB = kThreads / LPR;
  // One lane per row (D == CPL): a lane's row is a D-float stride in memory, so
  // the block's rows -- one contiguous run of nrows * D floats -- go through an
  // LDS tile (odd row stride TS: no bank conflicts) and move as coalesced
  // 4-byte-per-lane sweeps.  Every loop bound below is block-uniform, so every
  // thread reaches every barrier.
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
      planar_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
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

// Calibrator.predict of a planar flow calibrator (calibrators.py:40-44,
// 330-353), the row in registers from load to store: centre on the mean of the
// D real columns, run the stack, p = softmax(z), then
// softmax(log(p + 1e-7) - log_priors).  Padding columns (c >= D) hold 0 through
// the stack (their w and u_hat are 0) and enter no mean, maximum or sum.  A
// -inf log-prior makes q = +inf, q - max = NaN and the row's sum NaN: the whole
// row is NaN, as the reference's is.  Same grid, tile and barriers as
// k_planar_fwd.
template <int LPR, int CPL>
__global__ __launch_bounds__(kThreads) void k_planar_predict(
    const float* __restrict__ x, const float* __restrict__ blob, const float* __restrict__ lp,
    int D, int L, int cs, int64_t B, float* __restrict__ probs, float* __restrict__ ld_out) {
#define CNF_SCORE 0
#include "cnf_planar_predict.inc"
#undef CNF_SCORE
}

// k_planar_predict with the scoring epilogue (cnf_score.h) in place of the
// store phase; the log-det is not written
template <int LPR, int CPL>
__global__ __launch_bounds__(kThreads) void k_planar_score(
    const float* __restrict__ x, const float* __restrict__ blob, const float* __restrict__ lp,
    int D, int L, int cs, int64_t B, score::Args sc) {
  __shared__ long long rec[score::kRecWords];
#define CNF_SCORE 1
#include "cnf_planar_predict.inc"
#undef CNF_SCORE
}

// ---- reverse mode -------------------------------------------------------------

struct BwdArgs {
  const float* x;
  const float* blob;
  const int64_t* y;     // non-null: the fused loss seeds the sweep
  const float* gz;      // upstream gradients (y == null), each may be null
  const float* gz_all;
  const float* gld;
  float* dx;
  float* part;          // block records (wave records when gacc)
  float* tape;          // [L][B] when L > kRegL
  int64_t B;
  int D, L, cs, ps, pw, gacc, kind;
  float det, gscale;
};

// Backward through layer l.  In: xv = z_l, g = gradient at z_l, h.  Out: xv =
// x_l, g = gradient at x_l; con[] = this row's 2 CPL + 2 contributions
// [h g | g_a x_l | G_c, G_b].
template <int LPR, int CPL>
__device__ __forceinline__ void planar_back(float* xv, float* g, float h, float gam, bool valid,
                                            const float* __restrict__ cb, int gl, float* con) {
  constexpr int DP = LPR * CPL;
  const float c = cb[2 * DP + 1];
  const float hp = 1.f - h * h;
  const float q = 1.f + hp * c;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const float uh = cb[DP + gl + LPR * k];
    xv[k] = fmaf(-h, uh, xv[k]);
    s = fmaf(g[k], uh, s);
  }
  s = row_sum<LPR>(s);
  float ga = s * hp + gam * (c / q) * (-2.f * h * hp);
  float gc = gam * hp / q;
  if (!valid) ga = gc = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    con[k] = h * g[k];
    con[CPL + k] = ga * xv[k];
    g[k] = fmaf(ga, cb[gl + LPR * k], g[k]);
  }
  con[2 * CPL] = gc;
  con[2 * CPL + 1] = ga;
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

template <int LPR, int CPL, bool REGT, bool REGA>
__global__ __launch_bounds__(kThreads) void k_planar_bwd(BwdArgs A) {
  constexpr int RPB = kThreads / LPR;
  constexpr int NW = 2 * CPL + 2;
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
    float ht[REGT ? kRegL : 1];
    float ld = 0.f;
    if constexpr (REGT) {
#pragma unroll
      for (int l = 0; l < kRegL; ++l)
        if (l < L) ht[l] = planar_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
    } else {
      for (int l = 0; l < L; ++l) {
        const float h = planar_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
        if (valid && gl == 0) A.tape[(int64_t)l * B + row] = h;
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
      for (int l = kRegL - 1; l >= 0; --l) {
        if (l < L) {
          planar_back<LPR, CPL>(xv, g, ht[l], gam, valid, blob + (size_t)l * cs, gl, con);
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
        float h = 0.f;
        if (valid && gl == 0) h = A.tape[(int64_t)l * B + row];  // the lane that wrote it
        h = __shfl(h, lane - gl);
        planar_back<LPR, CPL>(xv, g, h, gam, valid, blob + (size_t)l * cs, gl, con);
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
// writes the three loss terms, then applies the chain rule through u_hat per
// layer and writes the flat gradient.
__global__ __launch_bounds__(kFinThreads) void k_planar_finish(
    const float* __restrict__ part, int units, int pw, int nsum, float* __restrict__ sums,
    float* __restrict__ terms, float* __restrict__ grads, const float* __restrict__ blob, Ptrs P,
    int D, int L, int dp, int cs) {
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
    const float* cb = blob + (size_t)l * cs;
    const float* S = sums + (size_t)l * ps;
    const float* u = P.p[3 * l + 1];
    float* go = grads + (size_t)l * (2 * D + 1);
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
  }
}

// ---- launches -------------------------------------------------------------------

// What cnf_rowflow.h's launch layer asks of a family.
struct Planar {
  using Table = Ptrs;
  using Args = BwdArgs;
  static constexpr bool kLdScalar = false;  // the log-det is a row's: [B]
  static const RowFamily& family() { return kFamily; }
  static constexpr int grad_floats(int D, int = 0) { return 2 * D + 1; }  // w, u, b
  static int8_t* kinds(Ptrs&) { return nullptr; }

  static void prep(const Ptrs& P, const Geo& g, int D, int L, float* blob, bool, hipStream_t s) {
    hipLaunchKernelGGL(k_planar_prep, dim3(L), dim3(64), 0, s, P, blob, D, g.dp, g.cs);
  }

  template <int LPR, int CPL>
  static void fwd(int blocks, const FwdCall& c, const Geo& g, const float* blob, float* part) {
    hipLaunchKernelGGL((k_planar_fwd<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x, blob,
                       c.D, c.L, g.cs, c.B, c.z, c.ld, c.z_all, c.y, c.kind, c.det, part);
  }

  template <int LPR, int CPL>
  static void predict(int blocks, const PredictCall& c, const Geo& g, const float* blob,
                      const score::Args* sc) {
    if (sc) {
      hipLaunchKernelGGL((k_planar_score<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x,
                         blob, c.lp, c.D, c.L, g.cs, c.B, *sc);
    } else {
      hipLaunchKernelGGL((k_planar_predict<LPR, CPL>), dim3(blocks), dim3(kThreads), 0, c.s, c.x,
                         blob, c.lp, c.D, c.L, g.cs, c.B, c.probs, c.ld);
    }
  }

  template <int LPR, int CPL>
  static void bwd(int blocks, size_t lds, hipStream_t s, const BwdArgs& a) {
    if (!planar_bwd_variant(LPR, CPL, a.L).regt) {
      hipLaunchKernelGGL((k_planar_bwd<LPR, CPL, false, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
      return;
    }
    // rega depends on the depth through regt alone: the geometry's answer at kRegL
    if constexpr (planar_bwd_variant(LPR, CPL, kRegL).rega) {
      hipLaunchKernelGGL((k_planar_bwd<LPR, CPL, true, true>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
    } else {
      hipLaunchKernelGGL((k_planar_bwd<LPR, CPL, true, false>), dim3(blocks), dim3(kThreads), lds,
                         s, a);
    }
  }

  static void fill(BwdArgs& a, const BwdCall& c, float* tape) {
    a.gld = c.loss ? nullptr : c.gld;
    a.tape = tape;
    a.det = c.det;
  }

  static void finish(const Finish& f, const Ptrs& P, int D, int L, const Geo& g, const BwdCall*,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_planar_finish, dim3(1), dim3(kFinThreads), 0, s, f.part, f.units, f.pw,
                       f.nsum, f.sums, f.terms, f.grads, f.blob, P, D, L, g.dp, g.cs);
  }
};

}  // namespace
}  // namespace cnf

extern "C" int cnf_planar_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats) {
  return cnf::rowflow::param_count(cnf::kFamily, cnf::Planar::grad_floats, dim, n_layers, n_floats);
}

extern "C" int cnf_planar_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B,
                                          size_t* bytes) {
  return cnf::rowflow::workspace_bytes(cnf::kFamily, dim, n_layers, B, bytes);
}

extern "C" int cnf_planar_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]) {
  return cnf::rowflow::launch_plan(cnf::kFamily, dim, n_layers, B, out);
}

extern "C" int cnf_planar_forward(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, float* z, float* logdet, float* z_all, int64_t B,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_planar_forward");
  return cnf::rowflow::run_forward<cnf::Planar>({dim, n_layers, params, x, nullptr, 0, 0.f, z,
                                                 logdet, z_all, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false,
                                                 false});
}

extern "C" int cnf_planar_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                                       const float* x, const int64_t* y, int32_t loss_kind,
                                       float det, float* z, float* logdet, float* loss_terms,
                                       int64_t B, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  CNF_RANGE("cnf_planar_forward_loss");
  return cnf::rowflow::run_forward<cnf::Planar>({dim, n_layers, params, x, y, loss_kind, det, z,
                                                 logdet, nullptr, loss_terms, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true,
                                                 false});
}

extern "C" int cnf_planar_predict(int32_t dim, int32_t n_layers, const float* const* params,
                                  const float* x, const float* log_priors, float* probs,
                                  float* logdet, int64_t B, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_planar_predict");
  return cnf::rowflow::run_predict<cnf::Planar>({dim, n_layers, params, x, log_priors, probs,
                                                 logdet, nullptr, 0, nullptr, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, false});
}

extern "C" int cnf_planar_score(int32_t dim, int32_t n_layers, const float* const* params,
                                const float* x, const float* log_priors, const int64_t* y,
                                int32_t bins, int64_t* record, int64_t B, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_planar_score");
  return cnf::rowflow::run_predict<cnf::Planar>({dim, n_layers, params, x, log_priors, nullptr,
                                                 nullptr, y, bins, record, B, workspace,
                                                 workspace_bytes, (hipStream_t)stream, true});
}

extern "C" int cnf_planar_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                              const float* x, const float* gz, const float* gz_all,
                              const float* gld, float* grads, float* dx, int64_t B, void* workspace,
                              size_t workspace_bytes, void* stream) {
  CNF_RANGE("cnf_planar_vjp");
  return cnf::rowflow::run_backward<cnf::Planar>({dim, n_layers, params, x, nullptr, 0, 0.f, 1.f,
                                                  gz, gz_all, gld, nullptr, grads, dx, B, workspace,
                                                  workspace_bytes, (hipStream_t)stream, false});
}

extern "C" int cnf_planar_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                                   const float* x, const int64_t* y, int32_t loss_kind, float det,
                                   float grad_scale, float* loss_terms, float* grads, float* dx,
                                   int64_t B, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  CNF_RANGE("cnf_planar_loss_vjp");
  return cnf::rowflow::run_backward<cnf::Planar>({dim, n_layers, params, x, y, loss_kind, det,
                                                  grad_scale, nullptr, nullptr, nullptr, loss_terms,
                                                  grads, dx, B, workspace, workspace_bytes,
                                                  (hipStream_t)stream, true});
}
