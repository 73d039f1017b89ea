// What the row-wise flow families (cnf_planar.hip, cnf_radial.hip,
// cnf_affine.hip, cnf_mixed.hip) share: the grid constants, the geometry of a
// row in lanes, the workspace plan, the shape dispatch, the lane helpers, and the whole host layer
// between the extern "C" entry points and the launches: the argument checks
// and their order, the B == 0 contract, the prep launch, the choice between
// workspace and LDS records, the finish launch and the status tail
// (run_forward, run_predict, run_backward).
// A family differs from the others in three geometry words -- cs, the floats of
// its per-layer constant record, ps, the row sums per layer of its reverse
// mode, and tf, the tape floats per (row, layer) its deep stacks keep in the
// workspace (1, or 0 for a family without such a tape) -- which it passes to
// geometry(), in its parameter tensors per layer (RowFamily::tensors), and in
// what its policy type says (below, "the launch layer"): its kernels'
// argument lists and the gradient floats of a layer.  The mixed family's layers
// differ in kind: its calls carry `kinds`, checked directly after the shape,
// and a layer's tensors and gradient floats go by its kind
// (RowFamily::kind_tensors, grad_floats(D, kind)).
//
// Everything here is either host code or an inline device function that was
// one already; the kernel bodies stay in their files, because wrapping kernel
// text in a helper makes the compiler schedule it differently.
// `Ptrs`, the by-value pointer table of the prep and finish kernels, and
// `BwdArgs` stay in each file too: their namespace is part of those kernels'
// names.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cnf_internal.h"
#include "cnf_score.h"

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

// Which instantiation of a family's reverse-mode kernel a launch takes: regt,
// the tape in registers (L <= kRegL); rega, per-lane accumulators on top of it
// (the family says for which geometries).  One helper per family answers it,
// for its policy's bwd launcher and for cnf_<family>_launch_plan alike.
struct BwdVariant {
  bool regt, rega;
};

// A family: its layer cap, its geometry(D, L, cs, ps, tf) with the family words
// filled in, its reverse-mode variant for a geometry and depth, and its
// parameter tensors per layer.  A family whose layers differ in kind (mixed)
// also says how many of those tensors a layer of a kind has; its calls then
// carry `kinds`, and the caller's table is packed by those counts.
struct RowFamily {
  int max_layers;
  Geo (*geo)(int D, int L);
  BwdVariant (*bwd)(int lpr, int cpl, int L);
  int tensors = 3;
  int (*kind_tensors)(int kind) = nullptr;
};

// What every entry point checks first: the shape, then, for a family that
// takes them, `kinds` null and each of its values in order.
static inline int check_head(const RowFamily& f, int32_t dim, int32_t n_layers,
                             const int32_t* kinds) {
  if (dim < 1 || n_layers < 1) return CNF_ERR_DESC;
  if (dim > CNF_MAX_DIM || n_layers > f.max_layers) return CNF_ERR_UNSUPPORTED;
  if (!f.kind_tensors) return CNF_OK;
  if (!kinds) return CNF_ERR_NULL;
  for (int l = 0; l < n_layers; ++l)
    if (kinds[l] < CNF_LAYER_PLANAR || kinds[l] > CNF_LAYER_AFFINE) return CNF_ERR_DESC;
  return CNF_OK;
}

// Common argument checks; fills the pointer table (tensors slots per layer,
// max_layers layers; null where the layer has no such tensor or is not given),
// the table's kinds (`kd`, null for a family of one kind; 0 past n_layers), the
// geometry and the plan.  The caller's table is read entry by entry and no
// further than the layers' tensors add up to.
static inline int check_common(const RowFamily& f, int32_t dim, int32_t n_layers,
                               const int32_t* kinds, const float* const* params, const float* x,
                               int64_t B, const void* ws, size_t ws_bytes, const float** table,
                               int8_t* kd, Geo* g, Plan* p) {
  const int st = check_head(f, dim, n_layers, kinds);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  if (!params) return CNF_ERR_NULL;
  const int nt = f.tensors;
  for (int l = 0, i = 0; l < f.max_layers; ++l) {
    const int n = l >= n_layers ? 0 : f.kind_tensors ? f.kind_tensors(kinds[l]) : nt;
    if (kd) kd[l] = l < n_layers ? (int8_t)kinds[l] : 0;
    for (int j = 0; j < nt; ++j) {
      const float* q = nullptr;
      if (j < n) {
        q = params[i++];
        if (!q) return CNF_ERR_NULL;
        if (mis4(q)) return CNF_ERR_ALIGN;
      }
      table[nt * l + j] = q;
    }
  }
  *g = f.geo(dim, n_layers);
  *p = plan(*g, n_layers, B);
  if (B > 0 && (!x || !ws || ws_bytes < (size_t)p->total * sizeof(float))) return CNF_ERR_NULL;
  if (mis4(x) || mis4(ws)) return CNF_ERR_ALIGN;
  return CNF_OK;
}

// the body of cnf_<family>_workspace_bytes
inline int workspace_bytes(const RowFamily& f, int32_t dim, int32_t n_layers, int64_t B,
                           size_t* bytes, const int32_t* kinds = nullptr) {
  if (!bytes) return CNF_ERR_NULL;
  const int st = check_head(f, dim, n_layers, kinds);
  if (st != CNF_OK) return st;
  if (B < 0 || B > kMaxRows) return CNF_ERR_BATCH;
  *bytes = (size_t)plan(f.geo(dim, n_layers), n_layers, B).total * sizeof(float);
  return CNF_OK;
}

// the body of cnf_<family>_launch_plan: what a call of this shape would launch,
// from the functions the launches themselves use.  Host only.
inline int launch_plan(const RowFamily& f, int32_t dim, int32_t n_layers, int64_t B,
                       int32_t* out, const int32_t* kinds = nullptr) {
  if (!out) return CNF_ERR_NULL;
  const int st = check_head(f, dim, n_layers, kinds);
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

// gradient (= parameter) floats of a stack: the sum over its layers, each of
// its kind (kind 0 where the family has one kind and `kinds` is null)
static inline int64_t grad_total(int (*grad_floats)(int D, int kind), int D, int L,
                                 const int32_t* kinds) {
  int64_t n = 0;
  for (int l = 0; l < L; ++l) n += grad_floats(D, kinds ? kinds[l] : 0);
  return n;
}

// the body of cnf_<family>_param_count
static inline int param_count(const RowFamily& f, int (*grad_floats)(int D, int kind), int32_t dim,
                              int32_t n_layers, int64_t* n_floats,
                              const int32_t* kinds = nullptr) {
  if (!n_floats) return CNF_ERR_NULL;
  const int st = check_head(f, dim, n_layers, kinds);
  if (st != CNF_OK) return st;
  *n_floats = grad_total(grad_floats, dim, n_layers, kinds);
  return CNF_OK;
}

// ---- the launch layer -------------------------------------------------------------
//
// One record per kind of call, with every argument any family has; an entry
// point whose family lacks one passes null / 0 (mis4(nullptr) is false, so one
// alignment line serves all; `kinds`, the last word of each record, is null
// unless the family's layers differ in kind).  run_forward, run_predict and
// run_backward own the order of the checks, which is part of the ABI
// (DESIGN.md 7k states it).
// A family's policy type F, defined in its file's anonymous namespace, supplies
//   Table, Args             its Ptrs (mixed: its Ptrs and Kinds) and BwdArgs
//   family()                its RowFamily
//   grad_floats(D, kind)    gradient (= parameter) floats of a layer
//   kinds(P)                the table's kinds, int8_t[max_layers]; null for one kind
//   kLdScalar               whether the log-det is one number [1], not a row's [B]
//   prep(P, g, D, L, blob, inv, s)                 the constant-record launch
//   fwd / predict / bwd <LPR, CPL>(...)            its kernels' launches
//   fill(a, call, tape)     the words of Args only this family has
//   finish(f, P, D, L, g, call, s)                 the one-block reduction's launch

struct FwdCall {
  int32_t D, L;
  const float* const* params;
  const float* x;
  const int64_t* y;  // null unless loss
  int32_t kind;
  float det;
  float *z, *ld, *z_all, *terms;
  int64_t B;
  void* ws;
  size_t ws_bytes;
  hipStream_t s;
  bool loss, inv;
  const int32_t* kinds = nullptr;
};

struct PredictCall {
  int32_t D, L;
  const float* const* params;
  const float *x, *lp;
  float *probs, *ld;
  const int64_t* y;  // scoring: labels, bins, record
  int32_t bins;
  int64_t* record;
  int64_t B;
  void* ws;
  size_t ws_bytes;
  hipStream_t s;
  bool scoring;
  const int32_t* kinds = nullptr;
};

struct BwdCall {
  int32_t D, L;
  const float* const* params;
  const float* x;
  const int64_t* y;
  int32_t kind;
  float det, gscale;
  const float *gz, *gz_all, *gld;
  float *terms, *grads, *dx;
  int64_t B;
  void* ws;
  size_t ws_bytes;
  hipStream_t s;
  bool loss;
  const int32_t* kinds = nullptr;
};

// What a finish launch adds up: `units` records of `pw` words at `part`, the
// first `nsum` of them row sums (to `sums`), the next three the loss terms.
struct Finish {
  const float* part;
  int units, pw, nsum;
  float *sums, *terms, *grads;
  const float* blob;
};

static inline int check_loss(int32_t kind, const int64_t* y, const float* terms, int64_t B) {
  if (kind != CNF_LOSS_CAL && kind != CNF_LOSS_CE) return CNF_ERR_DESC;
  if (!terms || (B > 0 && !y)) return CNF_ERR_NULL;
  if (mis8(y) || mis4(terms)) return CNF_ERR_ALIGN;
  return CNF_OK;
}

static inline int zero_floats(float* p, size_t n, hipStream_t s) {
  return hip_status(hipMemsetAsync(p, 0, n * sizeof(float), s));
}

// forward, forward + loss (c.loss), inverse (c.inv)
template <class F>
int run_forward(const FwdCall& c) {
  typename F::Table P;
  Geo g;
  Plan p;
  int st = check_common(F::family(), c.D, c.L, c.kinds, c.params, c.x, c.B, c.ws, c.ws_bytes, P.p,
                        F::kinds(P), &g, &p);
  if (st != CNF_OK) return st;
  if (c.loss && (st = check_loss(c.kind, c.y, c.terms, c.B)) != CNF_OK) return st;
  if (mis4(c.z) || mis4(c.ld) || mis4(c.z_all)) return CNF_ERR_ALIGN;
  if (c.B == 0) {  // no row: the terms are 0; a [1] log-det is not formed without a launch
    if (c.loss) st = zero_floats(c.terms, 3, c.s);
    if (st == CNF_OK && F::kLdScalar && c.ld) st = zero_floats(c.ld, 1, c.s);
    return st;
  }
  float* w = static_cast<float*>(c.ws);
  F::prep(P, g, c.D, c.L, w + p.blob, c.inv, c.s);
  st = launch_status();
  if (st != CNF_OK) return st;
  const int blocks = fwd_blocks(g, c.B);
  float* part = c.loss ? w + p.part : nullptr;
  CNF_ROWFLOW_DISPATCH(F::template fwd, blocks, c, g, w + p.blob, part);
  st = launch_status();
  if (st != CNF_OK || !c.loss) return st;
  F::finish(Finish{part, blocks, 4, 0, w + p.sums, c.terms, nullptr, w + p.blob}, P, c.D, c.L, g,
            nullptr, c.s);
  return launch_status();
}

// predict, or score (c.scoring)
template <class F>
int run_predict(const PredictCall& c) {
  typename F::Table P;
  Geo g;
  Plan p;
  int st = check_head(F::family(), c.D, c.L, c.kinds);
  if (st != CNF_OK) return st;
  if (c.scoring && (st = score::check_args(c.D, c.bins, c.B, c.y, c.record)) != CNF_OK) return st;
  st = check_common(F::family(), c.D, c.L, c.kinds, c.params, c.x, c.B, c.ws, c.ws_bytes, P.p,
                    F::kinds(P), &g, &p);
  if (st != CNF_OK) return st;
  if (c.B > 0 && (!c.lp || (!c.scoring && !c.probs))) return CNF_ERR_NULL;
  if (mis4(c.lp) || mis4(c.probs) || mis4(c.ld)) return CNF_ERR_ALIGN;
  if (c.B == 0) return CNF_OK;
  float* w = static_cast<float*>(c.ws);
  F::prep(P, g, c.D, c.L, w + p.blob, false, c.s);
  st = launch_status();
  if (st != CNF_OK) return st;
  score::Args sc;
  if (c.scoring) sc = score::make_args(c.y, c.bins, c.record);
  CNF_ROWFLOW_DISPATCH(F::template predict, fwd_blocks(g, c.B), c, g, w + p.blob,
                       c.scoring ? &sc : nullptr);
  return launch_status();
}

// reverse mode from upstream gradients, or fused with the loss (c.loss)
template <class F>
int run_backward(const BwdCall& c) {
  typename F::Table P;
  Geo g;
  Plan p;
  int st = check_common(F::family(), c.D, c.L, c.kinds, c.params, c.x, c.B, c.ws, c.ws_bytes, P.p,
                        F::kinds(P), &g, &p);
  if (st != CNF_OK) return st;
  if (!c.grads) return CNF_ERR_NULL;
  if (c.loss && (st = check_loss(c.kind, c.y, c.terms, c.B)) != CNF_OK) return st;
  if (mis4(c.gz) || mis4(c.gz_all) || mis4(c.gld) || mis4(c.grads) || mis4(c.dx))
    return CNF_ERR_ALIGN;
  if (c.B == 0) {
    st = zero_floats(c.grads, (size_t)grad_total(F::grad_floats, c.D, c.L, c.kinds), c.s);
    if (st == CNF_OK && c.loss) st = zero_floats(c.terms, 3, c.s);
    return st;
  }
  float* w = static_cast<float*>(c.ws);
  F::prep(P, g, c.D, c.L, w + p.blob, false, c.s);
  st = launch_status();
  if (st != CNF_OK) return st;
  const int blocks = bwd_blocks(g, c.B);
  const int units = bwd_units(g, c.B);
  size_t lds = 0;
  if (g.gacc) {
    st = zero_floats(w + p.part, (size_t)units * g.pw, c.s);
    if (st != CNF_OK) return st;
  } else {
    lds = (size_t)kWaves * g.pw * sizeof(float);
  }
  typename F::Args a;  // the words every family's BwdArgs has, then its own
  a.x = c.x;
  a.blob = w + p.blob;
  a.y = c.loss ? c.y : nullptr;
  a.gz = c.loss ? nullptr : c.gz;
  a.gz_all = c.loss ? nullptr : c.gz_all;
  a.dx = c.dx;
  a.part = w + p.part;
  a.B = c.B;
  a.D = c.D;
  a.L = c.L;
  a.cs = g.cs;
  a.ps = g.ps;
  a.pw = g.pw;
  a.gacc = g.gacc ? 1 : 0;
  a.kind = c.kind;
  a.gscale = c.gscale;
  F::fill(a, c, w + p.tape);
  CNF_ROWFLOW_DISPATCH(F::template bwd, blocks, lds, c.s, a);
  st = launch_status();
  if (st != CNF_OK) return st;
  F::finish(Finish{a.part, units, g.pw, c.L * g.ps, w + p.sums, c.loss ? c.terms : nullptr, c.grads,
                   w + p.blob},
            P, c.D, c.L, g, &c, c.s);
  return launch_status();
}

}  // namespace rowflow
}  // namespace cnf
