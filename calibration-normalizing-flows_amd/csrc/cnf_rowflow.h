// What the row-wise flow families (cnf_planar.hip, cnf_radial.hip,
// cnf_affine.hip) share: the grid constants, the geometry of a row in lanes, the
// workspace plan, the argument checks, the shape dispatch and the lane helpers.
// A family differs from the others in three geometry words -- cs, the floats of
// its per-layer constant record, ps, the row sums per layer of its reverse
// mode, and tf, the tape floats per (row, layer) its deep stacks keep in the
// workspace (1, or 0 for a family without such a tape) -- which it passes to
// geometry(), and in its parameter tensors per layer (RowFamily::tensors).
//
// Everything here is either host code or an inline device function that was
// one already; the kernel bodies stay in their files, because wrapping kernel
// text in a helper makes the compiler schedule it differently.
// `Ptrs`, the by-value pointer table of the prep and finish kernels, stays in
// each file too: its namespace is part of those kernels' names.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cnf_internal.h"

namespace cnf {
namespace rowflow {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRegL = 10;        // tape in registers / per-lane accumulators up to this depth
constexpr int kFwdCap = 1024;    // grid caps in blocks
constexpr int kBwdCap = 256;
constexpr int kLdsWords = 3072;  // a wave's record in LDS up to this many floats (4 x 12 KB)
constexpr int kFinThreads = 1024;
constexpr int64_t kMaxRows = (int64_t)1 << 31;

// Rows: one lane per row for D <= 16, 16 lanes per row for D <= 64, 64 above;
// column c of a row sits in lane c % lpr, slot c / lpr (cpl slots, dp = lpr * cpl).
struct Geo {
  int lpr, cpl, dp, cs, ps, pw, tf;
  bool gacc;
};

inline int lanes_per_row(int D) { return D <= 16 ? 1 : D <= 64 ? 16 : 64; }

// D rounded up to a whole number of slots per lane
inline int padded_dim(int D) {
  const int lpr = lanes_per_row(D);
  return (D + lpr - 1) / lpr * lpr;
}

inline Geo geometry(int D, int L, int cs, int ps, int tf = 1) {
  Geo g;
  g.lpr = lanes_per_row(D);
  g.dp = padded_dim(D);
  g.cpl = g.dp / g.lpr;
  g.cs = cs;
  g.ps = ps;
  g.pw = L * g.ps + 4;
  g.tf = tf;
  g.gacc = g.pw > kLdsWords;
  return g;
}

inline int64_t round64(int64_t n) { return (n + 63) / 64 * 64; }

inline int fwd_blocks(const Geo& g, int64_t B) {
  const int64_t rpb = kThreads / g.lpr;
  const int64_t n = (B + rpb - 1) / rpb;
  return (int)(n < 1 ? 1 : n > kFwdCap ? kFwdCap : n);
}

inline int bwd_blocks(const Geo& g, int64_t B) {
  const int64_t rpb = kThreads / g.lpr;
  int64_t cap = kBwdCap;
  if (g.gacc) {
    cap = ((int64_t)1 << 20) / g.pw;
    cap = cap < 4 ? 4 : cap > kBwdCap ? kBwdCap : cap;
  }
  const int64_t n = (B + rpb - 1) / rpb;
  return (int)(n < 1 ? 1 : n > cap ? cap : n);
}

inline int bwd_units(const Geo& g, int64_t B) {
  return bwd_blocks(g, B) * (g.gacc ? kWaves : 1);
}

struct Plan {
  int64_t blob, sums, part, tape, total;  // float offsets / count
};

inline Plan plan(const Geo& g, int L, int64_t B) {
  Plan p;
  p.blob = 0;
  p.sums = round64((int64_t)L * g.cs);
  p.part = p.sums + round64(g.pw);
  int64_t pf = (int64_t)bwd_units(g, B) * g.pw;
  const int64_t lf = (int64_t)fwd_blocks(g, B) * 4;
  if (lf > pf) pf = lf;
  p.tape = p.part + round64(pf);
  p.total = p.tape + (L > kRegL ? round64((int64_t)L * B * g.tf) : 0);
  return p;
}

// ---- lane helpers -----------------------------------------------------------

// sum / max over the LPR lanes of a row (every lane gets the result)
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int LPR>
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// sum over the wave's lanes that hold the same column slot (lane % LPR)
template <int LPR>
__device__ __forceinline__ float col_sum(float v) {
#pragma unroll
  for (int o = 32; o >= LPR; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// softmax of the row's final z: m, log-sum, and log p_y
template <int LPR, int CPL>
__device__ __forceinline__ void row_softmax(const float* xv, int gl, int D, int64_t yy, float& m,
                                            float& lse, float& lpy) {
  m = -INFINITY;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
    if (gl + LPR * k < D) m = fmaxf(m, xv[k]);
  m = row_max<LPR>(m);
  float se = 0.f, zy = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int c = gl + LPR * k;
    if (c < D) {
      se += expf(xv[k] - m);
      if (c == yy) zy = xv[k];
    }
  }
  se = row_sum<LPR>(se);
  zy = row_sum<LPR>(zy);
  lse = logf(se);
  lpy = zy - (m + lse);
}

// ---- host side ------------------------------------------------------------------

// hip_status, launch_status, mis4 and mis8 are cnf_internal.h's (the enclosing namespace)

// FN<LPR, CPL>(args...) for the geometry `g` in scope
#define CNF_ROWFLOW_DISPATCH(FN, ...)                    \
  do {                                                   \
    if (g.lpr == 1) {                                    \
      switch (g.cpl) {                                   \
        case 1: FN<1, 1>(__VA_ARGS__); break;            \
        case 2: FN<1, 2>(__VA_ARGS__); break;            \
        case 3: FN<1, 3>(__VA_ARGS__); break;            \
        case 4: FN<1, 4>(__VA_ARGS__); break;            \
        case 5: FN<1, 5>(__VA_ARGS__); break;            \
        case 6: FN<1, 6>(__VA_ARGS__); break;            \
        case 7: FN<1, 7>(__VA_ARGS__); break;            \
        case 8: FN<1, 8>(__VA_ARGS__); break;            \
        case 9: FN<1, 9>(__VA_ARGS__); break;            \
        case 10: FN<1, 10>(__VA_ARGS__); break;          \
        case 11: FN<1, 11>(__VA_ARGS__); break;          \
        case 12: FN<1, 12>(__VA_ARGS__); break;          \
        case 13: FN<1, 13>(__VA_ARGS__); break;          \
        case 14: FN<1, 14>(__VA_ARGS__); break;          \
        case 15: FN<1, 15>(__VA_ARGS__); break;          \
        default: FN<1, 16>(__VA_ARGS__); break;          \
      }                                                  \
    } else if (g.lpr == 16) {                            \
      switch (g.cpl) {                                   \
        case 2: FN<16, 2>(__VA_ARGS__); break;           \
        case 3: FN<16, 3>(__VA_ARGS__); break;           \
        default: FN<16, 4>(__VA_ARGS__); break;          \
      }                                                  \
    } else {                                             \
      switch (g.cpl) {                                   \
        case 2: FN<64, 2>(__VA_ARGS__); break;           \
        case 3: FN<64, 3>(__VA_ARGS__); break;           \
        default: FN<64, 4>(__VA_ARGS__); break;          \
      }                                                  \
    }                                                    \
  } while (0)

inline int check_shape(int32_t dim, int32_t n_layers, int max_layers) {
  if (dim < 1 || n_layers < 1) return CNF_ERR_DESC;
  if (dim > CNF_MAX_DIM || n_layers > max_layers) return CNF_ERR_UNSUPPORTED;
  return CNF_OK;
}

// Which instantiation of a family's reverse-mode kernel a launch takes: regt,
// the tape in registers (L <= kRegL); rega, per-lane accumulators on top of it
// (the family says for which geometries).  One helper per family answers it,
// for launch_bwd and for cnf_<family>_launch_plan alike.
struct BwdVariant {
  bool regt, rega;
};

// A family: its layer cap, its geometry(D, L, cs, ps, tf) with the family words
// filled in, its reverse-mode variant for a geometry and depth, and its
// parameter tensors per layer.
struct RowFamily {
  int max_layers;
  Geo (*geo)(int D, int L);
  BwdVariant (*bwd)(int lpr, int cpl, int L);
  int tensors = 3;
};

// Common argument checks; fills the pointer table (tensors * max_layers
// entries, null past the tensors * n_layers given), the geometry and the plan.
inline int check_common(const RowFamily& f, int32_t dim, int32_t n_layers,
                        const float* const* params, const float* x, int64_t B, const void* ws,
                        size_t ws_bytes, const float** table, Geo* g, Plan* p) {
  const int st = check_shape(dim, n_layers, f.max_layers);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!params) return CNF_ERR_NULL;
  const int nt = f.tensors;
  for (int i = 0; i < nt * n_layers; ++i) {
    if (!params[i]) return CNF_ERR_NULL;
    if (mis4(params[i])) return CNF_ERR_ALIGN;
    table[i] = params[i];
  }
  for (int i = nt * n_layers; i < nt * f.max_layers; ++i) table[i] = nullptr;
  *g = f.geo(dim, n_layers);
  *p = plan(*g, n_layers, B);
  if (B > 0 && (!x || !ws || ws_bytes < (size_t)p->total * sizeof(float))) return CNF_ERR_NULL;
  if (mis4(x) || mis4(ws)) return CNF_ERR_ALIGN;
  return CNF_OK;
}

// the body of cnf_<family>_workspace_bytes
inline int workspace_bytes(const RowFamily& f, int32_t dim, int32_t n_layers, int64_t B,
                           size_t* bytes) {
  if (!bytes) return CNF_ERR_NULL;
  const int st = check_shape(dim, n_layers, f.max_layers);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  *bytes = (size_t)plan(f.geo(dim, n_layers), n_layers, B).total * sizeof(float);
  return CNF_OK;
}

// the body of cnf_<family>_launch_plan: what a call of this shape would launch,
// from the functions the launches themselves use.  Host only.
inline int launch_plan(const RowFamily& f, int32_t dim, int32_t n_layers, int64_t B,
                       int32_t* out) {
  if (!out) return CNF_ERR_NULL;
  const int st = check_shape(dim, n_layers, f.max_layers);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  const Geo g = f.geo(dim, n_layers);
  const BwdVariant v = f.bwd(g.lpr, g.cpl, n_layers);
  out[0] = g.lpr;
  out[1] = g.cpl;
  out[2] = v.regt ? 1 : 0;
  out[3] = v.rega ? 1 : 0;
  out[4] = g.gacc ? 1 : 0;
  out[5] = fwd_blocks(g, B);
  out[6] = bwd_blocks(g, B);
  out[7] = bwd_units(g, B);
  return CNF_OK;
}

}  // namespace rowflow
}  // namespace cnf
