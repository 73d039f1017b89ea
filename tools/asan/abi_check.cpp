// Host-side AddressSanitizer check of the C ABI's descriptor validation
// (sanitizers on host code only -- GPU ASan is not
// available on this pool).  Built by `make -C calibration-normalizing-flows_amd/csrc
// asan` against libcnf_hip_asan.so (cnf_abi.hip's host code instrumented) and
// run by tests/test_asan.py in the build container, no GPU needed: every
// call below either validates and returns, or sizes plans on the host.
//
// Seeded random descriptors -- valid, out of range, malformed hidden widths,
// random_flip permutation tables with out-of-range / duplicate entries,
// unknown option bits -- each through every size query and every launching
// entry point with a rejected argument (negative batch, NULL blob), so ASan
// sees the validation code read exactly the caller's arrays: the permutation
// table is a heap block of exactly L*D int64s.  The row families' argument
// paths (cnf_rowflow.h's launch layer) follow the same pattern, below.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "cnf.h"

static int g_fail = 0;
#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "abi_check: %s failed (line %d)\n", #c, __LINE__); \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

static bool is_status(int st) { return st <= 0 && st >= -6; }

// ---- the row families (cnf_planar_*, cnf_radial_*, cnf_affine_*) ------------------
//
// Their common checks copy the caller's parameter table into a tensors *
// max_layers pointer table on the entry point's stack.  The table handed in
// is a heap block of exactly tensors * L pointers (one pointer when the shape
// is out of range and nothing may be read), so ASan sees both ends.  Every
// launching call carries exactly one fault that returns before any HIP call;
// the pointers are fake and never followed on the host.

struct RowArgs {
  int32_t dim, L;
  const float* const* params;
  const float* x;
  int64_t B;
  void* ws;
  size_t wb;
  int32_t kind, bins;
  float* grads;
};

enum { ROW_LOSS = 1, ROW_BWD = 2, ROW_SCORE = 4 };
struct RowEntry {
  int cat;
  int (*fn)(const RowArgs&);
};
struct RowFamilyAbi {
  int tensors, max_layers;
  int (*grad_floats)(int D);
  int (*param_count)(int32_t, int32_t, int64_t*);
  int (*workspace_bytes)(int32_t, int32_t, int64_t, size_t*);
  int (*launch_plan)(int32_t, int32_t, int64_t, int32_t*);
  std::vector<RowEntry> entries;
};

alignas(8) static float g_f[8];
alignas(8) static int64_t g_i[8];

static const RowFamilyAbi kPlanar = {
    3, CNF_PLANAR_MAX_LAYERS, [](int D) { return 2 * D + 1; }, cnf_planar_param_count,
    cnf_planar_workspace_bytes, cnf_planar_launch_plan,
    {{0, [](const RowArgs& a) {
        return cnf_planar_forward(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_LOSS, [](const RowArgs& a) {
        return cnf_planar_forward_loss(a.dim, a.L, a.params, a.x, g_i, a.kind, 1.f, g_f, g_f, g_f,
                                       a.B, a.ws, a.wb, nullptr);
      }},
     {0, [](const RowArgs& a) {
        return cnf_planar_predict(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_SCORE, [](const RowArgs& a) {
        return cnf_planar_score(a.dim, a.L, a.params, a.x, g_f, g_i, a.bins, g_i, a.B, a.ws, a.wb,
                                nullptr);
      }},
     {ROW_BWD, [](const RowArgs& a) {
        return cnf_planar_vjp(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.grads, g_f, a.B, a.ws, a.wb,
                              nullptr);
      }},
     {ROW_BWD | ROW_LOSS, [](const RowArgs& a) {
        return cnf_planar_loss_vjp(a.dim, a.L, a.params, a.x, g_i, a.kind, 1.f, 1.f, g_f, a.grads,
                                   g_f, a.B, a.ws, a.wb, nullptr);
      }}}};

static const RowFamilyAbi kRadial = {
    3, CNF_RADIAL_MAX_LAYERS, [](int D) { return D + 2; }, cnf_radial_param_count,
    cnf_radial_workspace_bytes, cnf_radial_launch_plan,
    {{0, [](const RowArgs& a) {
        return cnf_radial_forward(a.dim, a.L, a.params, a.x, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_LOSS, [](const RowArgs& a) {
        return cnf_radial_forward_loss(a.dim, a.L, a.params, a.x, g_i, a.kind, g_f, g_f, a.B, a.ws,
                                       a.wb, nullptr);
      }},
     {0, [](const RowArgs& a) {
        return cnf_radial_predict(a.dim, a.L, a.params, a.x, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_SCORE, [](const RowArgs& a) {
        return cnf_radial_score(a.dim, a.L, a.params, a.x, g_f, g_i, a.bins, g_i, a.B, a.ws, a.wb,
                                nullptr);
      }},
     {ROW_BWD, [](const RowArgs& a) {
        return cnf_radial_vjp(a.dim, a.L, a.params, a.x, g_f, g_f, a.grads, g_f, a.B, a.ws, a.wb,
                              nullptr);
      }},
     {ROW_BWD | ROW_LOSS, [](const RowArgs& a) {
        return cnf_radial_loss_vjp(a.dim, a.L, a.params, a.x, g_i, a.kind, 1.f, g_f, a.grads, g_f,
                                   a.B, a.ws, a.wb, nullptr);
      }}}};

static const RowFamilyAbi kAffine = {
    2, CNF_AFFINE_MAX_LAYERS, [](int D) { return 2 * D; }, cnf_affine_param_count,
    cnf_affine_workspace_bytes, cnf_affine_launch_plan,
    {{0, [](const RowArgs& a) {
        return cnf_affine_forward(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {0, [](const RowArgs& a) {
        return cnf_affine_inverse(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_LOSS, [](const RowArgs& a) {
        return cnf_affine_forward_loss(a.dim, a.L, a.params, a.x, g_i, a.kind, 1.f, g_f, g_f, g_f,
                                       a.B, a.ws, a.wb, nullptr);
      }},
     {0, [](const RowArgs& a) {
        return cnf_affine_predict(a.dim, a.L, a.params, a.x, g_f, g_f, a.B, a.ws, a.wb, nullptr);
      }},
     {ROW_SCORE, [](const RowArgs& a) {
        return cnf_affine_score(a.dim, a.L, a.params, a.x, g_f, g_i, a.bins, g_i, a.B, a.ws, a.wb,
                                nullptr);
      }},
     {ROW_BWD, [](const RowArgs& a) {
        return cnf_affine_vjp(a.dim, a.L, a.params, a.x, g_f, g_f, g_f, a.grads, g_f, a.B, a.ws, a.wb,
                              nullptr);
      }},
     {ROW_BWD | ROW_LOSS, [](const RowArgs& a) {
        return cnf_affine_loss_vjp(a.dim, a.L, a.params, a.x, g_i, a.kind, 1.f, 1.f, g_f, a.grads,
                                   g_f, a.B, a.ws, a.wb, nullptr);
      }}}};

// One seeded (dim, L, B), the three host queries, then every launching entry
// point once per fault.  `want` is the fault's own status; a shape or batch
// outside the envelope is rejected first, with a status of its own.
template <class Rng>
static void row_family_check(const RowFamilyAbi& f, Rng& rng) {
  auto U = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  const int32_t dim = U(0, 9) == 0 ? U(-3, 300) : U(1, CNF_MAX_DIM);
  const int32_t L = U(0, 5) == 0 ? f.max_layers : U(0, 9) == 0 ? U(-2, f.max_layers + 6) : U(1, 12);
  const int64_t B = U(0, 5) != 0 ? (int64_t)U(1, 1 << 20)
                    : U(0, 1)    ? -(int64_t)U(1, 9)
                                 : ((int64_t)1 << 31) + U(1, 9);
  const bool shape_ok = dim >= 1 && dim <= CNF_MAX_DIM && L >= 1 && L <= f.max_layers;
  const bool ok = shape_ok && B >= 0 && B <= ((int64_t)1 << 31);
  int64_t nf = -1;
  size_t need = 0;
  int32_t plan[8] = {0};
  const int sp = f.param_count(dim, L, &nf);
  EXPECT(is_status(sp) && (sp == CNF_OK) == shape_ok);
  if (shape_ok) EXPECT(nf == (int64_t)L * f.grad_floats(dim));
  const int sw = f.workspace_bytes(dim, L, B, &need);
  EXPECT(is_status(sw) && (sw == CNF_OK) == ok);
  const int sl = f.launch_plan(dim, L, B, plan);
  EXPECT(is_status(sl) && (sl == CNF_OK) == ok);
  if (ok) EXPECT(need > 0 && need % 256 == 0 && plan[0] * plan[1] >= dim && plan[5] >= 1);
  EXPECT(f.param_count(dim, L, nullptr) == CNF_ERR_NULL);
  EXPECT(f.workspace_bytes(dim, L, B, nullptr) == CNF_ERR_NULL);
  EXPECT(f.launch_plan(dim, L, B, nullptr) == CNF_ERR_NULL);

  const int n = shape_ok ? f.tensors * L : 1;
  auto table = [&] {  // fresh, of exactly n fake aligned pointers
    std::vector<const float*> t(n);
    for (int i = 0; i < n; ++i) t[i] = reinterpret_cast<const float*>((uintptr_t)4096 + 64 * i);
    return t;
  };
  const RowArgs good = {dim, L, nullptr, g_f, B, g_f, need, CNF_LOSS_CAL, 15, g_f};
  // cats: the entry points the fault reaches (0: all); score's own checks come
  // before the common ones, so it may answer a common fault with its batch cap
  auto run = [&](RowArgs a, const std::vector<const float*>* t, int cats, int want) {
    a.params = t ? t->data() : nullptr;
    for (const RowEntry& e : f.entries) {
      if (cats && !(e.cat & cats)) continue;
      const int st = e.fn(a);
      EXPECT(st < 0 && is_status(st));
      const bool capped = (e.cat & ROW_SCORE) && (dim < 2 || B > (1 << 26));
      if (ok && !capped) EXPECT(st == want);
    }
  };
  std::vector<const float*> t = table();
  run(good, nullptr, 0, CNF_ERR_NULL);                       // a null table
  const int at = U(0, 2) == 0 ? n - 1 : U(0, n - 1);         // ... entry, the last one included
  t[at] = nullptr;
  run(good, &t, 0, CNF_ERR_NULL);
  t = table();
  t[at] = reinterpret_cast<const float*>((uintptr_t)4098);
  run(good, &t, 0, CNF_ERR_ALIGN);
  t = table();
  RowArgs a = good;
  a.wb = need - 4;                                           // a short workspace
  run(a, &t, 0, CNF_ERR_NULL);
  a = good;
  a.x = reinterpret_cast<const float*>((const char*)g_f + 2);
  run(a, &t, 0, CNF_ERR_ALIGN);
  a = good;
  a.kind = U(2, 9);
  run(a, &t, ROW_LOSS, CNF_ERR_DESC);
  a = good;
  a.grads = nullptr;
  run(a, &t, ROW_BWD, CNF_ERR_NULL);
  a = good;
  a.bins = U(0, 1) ? -U(0, 3) : CNF_MAX_BINS + U(1, 9);
  run(a, &t, ROW_SCORE, CNF_ERR_DESC);
}

// ---- the mixed family (cnf_mixed_*) ----------------------------------------------
//
// As above with `kinds` after n_layers: a heap block of exactly L words (one
// when the shape is out of range and nothing may be read), seeded over the
// three layer kinds, and a packed pointer table of exactly 3 or 2 entries per
// layer.  Malformed kinds arrays (a value outside 0..2 at a seeded place, the
// last included) and a null one are rejected directly after the shape.

struct MixedArgs {
  RowArgs r;
  const int32_t* kinds;
};

static const std::vector<std::pair<int, int (*)(const MixedArgs&)>> kMixedEntries = {
    {0, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_forward(a.dim, a.L, m.kinds, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb,
                                nullptr);
     }},
    {ROW_LOSS, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_forward_loss(a.dim, a.L, m.kinds, a.params, a.x, g_i, a.kind, 1.f, g_f, g_f,
                                     g_f, a.B, a.ws, a.wb, nullptr);
     }},
    {0, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_predict(a.dim, a.L, m.kinds, a.params, a.x, g_f, g_f, g_f, a.B, a.ws, a.wb,
                                nullptr);
     }},
    {ROW_SCORE, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_score(a.dim, a.L, m.kinds, a.params, a.x, g_f, g_i, a.bins, g_i, a.B, a.ws,
                              a.wb, nullptr);
     }},
    {ROW_BWD, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_vjp(a.dim, a.L, m.kinds, a.params, a.x, g_f, g_f, g_f, a.grads, g_f, a.B,
                            a.ws, a.wb, nullptr);
     }},
    {ROW_BWD | ROW_LOSS, [](const MixedArgs& m) {
       const RowArgs& a = m.r;
       return cnf_mixed_loss_vjp(a.dim, a.L, m.kinds, a.params, a.x, g_i, a.kind, 1.f, 1.f, g_f,
                                 a.grads, g_f, a.B, a.ws, a.wb, nullptr);
     }}};

template <class Rng>
static void mixed_check(Rng& rng) {
  auto U = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  const int max_layers = CNF_MIXED_MAX_LAYERS;
  const int32_t dim = U(0, 9) == 0 ? U(-3, 300) : U(1, CNF_MAX_DIM);
  const int32_t L = U(0, 5) == 0 ? max_layers : U(0, 9) == 0 ? U(-2, max_layers + 6) : U(1, 12);
  const int64_t B = U(0, 5) != 0 ? (int64_t)U(1, 1 << 20)
                    : U(0, 1)    ? -(int64_t)U(1, 9)
                                 : ((int64_t)1 << 31) + U(1, 9);
  const bool shape_ok = dim >= 1 && dim <= CNF_MAX_DIM && L >= 1 && L <= max_layers;
  const bool ok = shape_ok && B >= 0 && B <= ((int64_t)1 << 31);
  const int nk = shape_ok ? L : 1;
  std::vector<int32_t> kinds(nk);  // exactly L words
  int n = 0;                       // entries of the packed table
  int64_t want_nf = 0;
  for (int l = 0; l < nk; ++l) {
    kinds[l] = U(0, 2);
    n += kinds[l] == CNF_LAYER_AFFINE ? 2 : 3;
    want_nf += kinds[l] == CNF_LAYER_PLANAR ? 2 * dim + 1 : kinds[l] == CNF_LAYER_RADIAL ? dim + 2
                                                                                         : 2 * dim;
  }
  std::vector<int32_t> bad = kinds;  // one value outside 0..2, the last place included
  bad[U(0, 2) == 0 ? nk - 1 : U(0, nk - 1)] = U(0, 1) ? 3 + U(0, 9) : -1 - U(0, 9);
  int64_t nf = -1;
  size_t need = 0;
  int32_t plan[8] = {0};
  const int sp = cnf_mixed_param_count(dim, L, kinds.data(), &nf);
  EXPECT(is_status(sp) && (sp == CNF_OK) == shape_ok);
  if (shape_ok) EXPECT(nf == want_nf);
  const int sw = cnf_mixed_workspace_bytes(dim, L, kinds.data(), B, &need);
  EXPECT(is_status(sw) && (sw == CNF_OK) == ok);
  const int sl = cnf_mixed_launch_plan(dim, L, kinds.data(), B, plan);
  EXPECT(is_status(sl) && (sl == CNF_OK) == ok);
  if (ok) EXPECT(need > 0 && need % 256 == 0 && plan[0] * plan[1] >= dim && plan[5] >= 1);
  EXPECT(cnf_mixed_param_count(dim, L, kinds.data(), nullptr) == CNF_ERR_NULL);
  EXPECT(cnf_mixed_workspace_bytes(dim, L, kinds.data(), B, nullptr) == CNF_ERR_NULL);
  EXPECT(cnf_mixed_launch_plan(dim, L, kinds.data(), B, nullptr) == CNF_ERR_NULL);
  if (shape_ok) {  // kinds directly after the shape, before the batch
    EXPECT(cnf_mixed_param_count(dim, L, nullptr, &nf) == CNF_ERR_NULL);
    EXPECT(cnf_mixed_param_count(dim, L, bad.data(), &nf) == CNF_ERR_DESC);
    EXPECT(cnf_mixed_workspace_bytes(dim, L, nullptr, B, &need) == CNF_ERR_NULL);
    EXPECT(cnf_mixed_workspace_bytes(dim, L, bad.data(), B, &need) == CNF_ERR_DESC);
    EXPECT(cnf_mixed_launch_plan(dim, L, nullptr, B, plan) == CNF_ERR_NULL);
    EXPECT(cnf_mixed_launch_plan(dim, L, bad.data(), B, plan) == CNF_ERR_DESC);
  }

  auto table = [&] {  // fresh, of exactly n fake aligned pointers
    std::vector<const float*> t(n);
    for (int i = 0; i < n; ++i) t[i] = reinterpret_cast<const float*>((uintptr_t)4096 + 64 * i);
    return t;
  };
  const RowArgs good = {dim, L, nullptr, g_f, B, g_f, need, CNF_LOSS_CAL, 15, g_f};
  // shape_only: the fault is answered before the batch is looked at
  auto run = [&](RowArgs a, const int32_t* k, const std::vector<const float*>* t, int cats,
                 int want, bool shape_only) {
    a.params = t ? t->data() : nullptr;
    for (const auto& e : kMixedEntries) {
      if (cats && !(e.first & cats)) continue;
      const int st = e.second(MixedArgs{a, k});
      EXPECT(st < 0 && is_status(st));
      const bool capped = (e.first & ROW_SCORE) && (dim < 2 || B > (1 << 26));
      if (shape_only ? shape_ok : (ok && !capped)) EXPECT(st == want);
    }
  };
  std::vector<const float*> t = table();
  run(good, nullptr, &t, 0, CNF_ERR_NULL, true);               // a null kinds array
  run(good, bad.data(), &t, 0, CNF_ERR_DESC, true);            // a malformed one
  run(good, bad.data(), nullptr, 0, CNF_ERR_DESC, true);       // ... before the table is read
  run(good, kinds.data(), nullptr, 0, CNF_ERR_NULL, false);    // a null table
  const int at = U(0, 2) == 0 ? n - 1 : U(0, n - 1);           // ... entry, the last one included
  t[at] = nullptr;
  run(good, kinds.data(), &t, 0, CNF_ERR_NULL, false);
  t = table();
  t[at] = reinterpret_cast<const float*>((uintptr_t)4098);
  run(good, kinds.data(), &t, 0, CNF_ERR_ALIGN, false);
  t = table();
  RowArgs a = good;
  a.wb = need - 4;                                             // a short workspace
  run(a, kinds.data(), &t, 0, CNF_ERR_NULL, false);
  a = good;
  a.x = reinterpret_cast<const float*>((const char*)g_f + 2);
  run(a, kinds.data(), &t, 0, CNF_ERR_ALIGN, false);
  a = good;
  a.kind = U(2, 9);
  run(a, kinds.data(), &t, ROW_LOSS, CNF_ERR_DESC, false);
  a = good;
  a.grads = nullptr;
  run(a, kinds.data(), &t, ROW_BWD, CNF_ERR_NULL, false);
  a = good;
  a.bins = U(0, 1) ? -U(0, 3) : CNF_MAX_BINS + U(1, 9);
  run(a, kinds.data(), &t, ROW_SCORE, CNF_ERR_DESC, false);
}

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 3000;
  std::mt19937_64 rng(20261018);
  auto U = [&](int lo, int hi) { return (int)std::uniform_int_distribution<int>(lo, hi)(rng); };
  EXPECT(cnf_abi_version() == CNF_ABI_VERSION);
  for (int st = -8; st <= 1; ++st) EXPECT(cnf_strerror(st) != nullptr);
  int n_ok = 0;
  for (int it = 0; it < iters; ++it) {
    cnf_desc d;
    std::memset(&d, 0, sizeof d);
    d.abi_version = U(0, 19) == 0 ? U(-3, 5) : CNF_ABI_VERSION;
    d.dim = U(0, 9) == 0 ? U(-4, 300) : U(2, 128);
    d.n_layers = U(0, 19) == 0 ? U(-2, 0) : U(1, 14);
    d.n_hidden = U(0, 19) == 0 ? U(-1, CNF_MAX_HIDDEN + 2) : U(0, 3);
    for (int i = 0; i < CNF_MAX_HIDDEN; ++i)
      d.hidden[i] = U(0, 29) == 0 ? U(-2, 700) : U(1, 160);
    d.scale = U(0, 29) == 0 ? 2 : U(0, 1);
    d.shift = U(0, 29) == 0 ? -1 : U(0, 1);
    d.strict_nan = U(0, 3) == 0;
    d.options = U(0, 9) == 0 ? U(0, 31) : (U(0, 3) == 0 ? CNF_OPT_NO_SGPR : 0);
    std::vector<int64_t>* perms = nullptr;
    if (d.dim >= 2 && d.dim <= CNF_MAX_DIM && d.n_layers >= 1 && U(0, 2) == 0) {
      perms = new std::vector<int64_t>((size_t)d.n_layers * d.dim);
      for (int l = 0; l < d.n_layers; ++l) {
        int64_t* p = perms->data() + (size_t)l * d.dim;
        for (int j = 0; j < d.dim; ++j) p[j] = j;
        std::shuffle(p, p + d.dim, rng);
        const int kind = U(0, 9);
        if (kind == 0) p[0] = -1;                                   // no perm on this layer
        else if (kind == 1) p[U(0, d.dim - 1)] = d.dim + U(0, 5);  // out of range
        else if (kind == 2) p[U(0, d.dim - 1)] = p[(U(1, d.dim - 1))];  // duplicate (maybe)
      }
      d.perms = perms->data();
    }
    int64_t nf = -1;
    int32_t nt = -1;
    size_t bytes = 0, ws = 0;
    const int s0 = cnf_param_count(&d, &nf);
    EXPECT(is_status(s0));
    EXPECT(is_status(cnf_param_tensor_count(&d, &nt)));
    const int s1 = cnf_prepared_bytes(&d, &bytes);
    EXPECT(is_status(s1));
    EXPECT(cnf_kernel_name(&d) != nullptr);
    EXPECT(cnf_vjp_kernel_name(&d) != nullptr);
    const int64_t B = U(0, 4) == 0 ? -U(1, 9) : (int64_t)U(0, 1 << 20);
    EXPECT(is_status(cnf_forward_loss_workspace_bytes(&d, B, &ws)));
    EXPECT(is_status(cnf_vjp_workspace_bytes(&d, B, &ws)));
    EXPECT(is_status(cnf_vjp_inverse_workspace_bytes(&d, B, &ws)));
    int32_t plan[CNF_VJP_PLAN_WORDS];
    EXPECT(is_status(cnf_vjp_launch_plan(&d, B, U(0, 1), plan)));
    if (s0 == CNF_OK) {
      ++n_ok;
      // an empty stack (no s- and no t-net) has no parameters
      const bool nets = d.scale || d.shift;
      EXPECT(nets ? (nf > 0 && nt > 0) : (nf == 0 && nt == 0));
      EXPECT(s1 == CNF_OK && bytes > 0);
    }
    // launching entry points with a rejected argument: no launch may happen
    float dummy[4] = {0, 0, 0, 0};
    const int64_t nb = -1 - U(0, 3);
    EXPECT(cnf_forward(&d, nullptr, dummy, dummy, dummy, nullptr, nb, nullptr) < 0);
    EXPECT(cnf_inverse(&d, nullptr, dummy, dummy, dummy, nullptr, 4, nullptr) < 0);
    EXPECT(cnf_forward_loss(&d, nullptr, dummy, nullptr, CNF_LOSS_CAL, 1.f, nullptr, nullptr,
                            dummy, 4, nullptr, 0, nullptr) < 0);
    EXPECT(cnf_predict(&d, nullptr, dummy, dummy, dummy, nullptr, nb, nullptr) < 0);
    EXPECT(cnf_vjp(&d, nullptr, dummy, nullptr, nullptr, nullptr, dummy, nullptr, nb, nullptr, 0,
                   nullptr) < 0);
    EXPECT(cnf_loss_vjp(&d, nullptr, dummy, nullptr, 7, 1.f, 1.f, dummy, dummy, nullptr, 4,
                        nullptr, 0, nullptr) < 0);
    EXPECT(cnf_vjp_inverse(&d, nullptr, dummy, nullptr, nullptr, nullptr, dummy, nullptr, nb,
                           nullptr, 0, nullptr) < 0);
    // (an empty stack -- no s- or t-net -- has nothing to update: CNF_OK, no launch)
    EXPECT(cnf_adam_step(&d, nullptr, dummy, dummy, dummy, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0,
                         nullptr) <= 0);
    EXPECT(cnf_guard_nonfinite(dummy, -1, nullptr, nullptr) < 0);
    // calibration scoring: size queries with random shapes, then the launching
    // entry point with one rejected argument each (range, batch, NULL, alignment)
    {
      const int32_t mdim = U(0, 4) == 0 ? U(-3, 400) : U(2, CNF_MAX_DIM);
      const int32_t mbins = U(0, 4) == 0 ? U(-3, 90) : U(1, CNF_MAX_BINS);
      const bool shape_ok = mdim >= 2 && mdim <= CNF_MAX_DIM && mbins >= 1 && mbins <= CNF_MAX_BINS;
      int64_t words = -1;
      size_t mws = 1;
      const int sw = cnf_metrics_record_words(mbins, &words);
      EXPECT(is_status(sw));
      EXPECT((sw == CNF_OK) == (mbins >= 1 && mbins <= CNF_MAX_BINS));
      if (sw == CNF_OK) EXPECT(words == 4 + 3 * (int64_t)mbins);
      const int sb = cnf_metrics_workspace_bytes(mdim, mbins, B, &mws);
      EXPECT(is_status(sb));
      EXPECT((sb == CNF_OK) == (shape_ok && B >= 0));
      if (sb == CNF_OK) EXPECT(mws == 0);
      EXPECT(cnf_metrics_workspace_bytes(mdim, mbins, B, nullptr) == CNF_ERR_NULL);
      alignas(8) int64_t lab[2] = {0, 0};
      alignas(8) int64_t rec[4 + 3 * CNF_MAX_BINS] = {0};
      const int sm = cnf_metrics(dummy, lab, mdim, mbins, nb, rec, nullptr, 0, nullptr);
      EXPECT(sm < 0 && is_status(sm));
      if (shape_ok) {
        EXPECT(sm == CNF_ERR_BATCH);
        EXPECT(cnf_metrics(dummy, lab, mdim, mbins, (1LL << 26) + 1, rec, nullptr, 0, nullptr) ==
               CNF_ERR_BATCH);
        EXPECT(cnf_metrics(nullptr, lab, mdim, mbins, 1, rec, nullptr, 0, nullptr) == CNF_ERR_NULL);
        EXPECT(cnf_metrics(dummy, nullptr, mdim, mbins, 1, rec, nullptr, 0, nullptr) == CNF_ERR_NULL);
        EXPECT(cnf_metrics(dummy, lab, mdim, mbins, 1, nullptr, nullptr, 0, nullptr) == CNF_ERR_NULL);
        EXPECT(cnf_metrics((const float*)((const char*)dummy + 2), lab, mdim, mbins, 1, rec, nullptr,
                           0, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_metrics(dummy, (const int64_t*)((const char*)lab + 4), mdim, mbins, 1, rec,
                           nullptr, 0, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_metrics(dummy, lab, mdim, mbins, 1, (int64_t*)((char*)rec + 4), nullptr, 0,
                           nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_metrics(nullptr, nullptr, mdim, mbins, 0, rec, nullptr, 0, nullptr) == CNF_OK);
        for (int64_t w : rec) EXPECT(w == 0);  // nothing was written
      }
    }
    // isotonic predict: one rejected argument each (range, batch, cap, NULL,
    // alignment); nothing may be launched or written
    {
      const int32_t pdim = U(0, 4) == 0 ? U(-3, 400) : U(2, CNF_MAX_DIM);
      const bool shape_ok = pdim >= 2 && pdim <= CNF_MAX_DIM;
      alignas(8) double tx[4] = {7, 7, 7, 7}, ty[4] = {7, 7, 7, 7}, lp[4] = {0, 0, 0, 0};
      alignas(8) int32_t nt[4] = {7, 7, 7, 7};
      float out[4] = {7, 7, 7, 7};
      const double* const odd = (const double*)((const char*)tx + 4);  // 4-aligned only
      const int sp = cnf_pav_predict(dummy, pdim, nb, tx, ty, nt, 1, lp, out, nullptr);
      EXPECT(sp < 0 && is_status(sp));
      if (shape_ok) {
        EXPECT(sp == CNF_ERR_BATCH);
        EXPECT(cnf_pav_predict(dummy, pdim, (1LL << 26) + 1, tx, ty, nt, 1, lp, out, nullptr) ==
               CNF_ERR_BATCH);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nt, 0, lp, out, nullptr) == CNF_ERR_DESC);
        EXPECT(cnf_pav_predict(nullptr, pdim, 1, tx, ty, nt, 1, lp, out, nullptr) == CNF_ERR_NULL);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, nullptr, ty, nt, 1, lp, out, nullptr) ==
               CNF_ERR_NULL);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, nullptr, nt, 1, lp, out, nullptr) ==
               CNF_ERR_NULL);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nullptr, 1, lp, out, nullptr) ==
               CNF_ERR_NULL);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nt, 1, nullptr, out, nullptr) ==
               CNF_ERR_NULL);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nt, 1, lp, nullptr, nullptr) ==
               CNF_ERR_NULL);
        EXPECT(cnf_pav_predict((const float*)((const char*)dummy + 2), pdim, 1, tx, ty, nt, 1, lp,
                               out, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, odd, ty, nt, 1, lp, out, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, odd, nt, 1, lp, out, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, (const int32_t*)((const char*)nt + 2), 1,
                               lp, out, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nt, 1, odd, out, nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(dummy, pdim, 1, tx, ty, nt, 1, lp, (float*)((char*)out + 2),
                               nullptr) == CNF_ERR_ALIGN);
        EXPECT(cnf_pav_predict(nullptr, pdim, 0, tx, ty, nt, 1, lp, nullptr, nullptr) == CNF_OK);
      }
      for (int k = 0; k < 4; ++k) EXPECT(tx[k] == 7 && ty[k] == 7 && nt[k] == 7 && out[k] == 7);
    }
    delete perms;
    for (const RowFamilyAbi* f : {&kPlanar, &kRadial, &kAffine}) row_family_check(*f, rng);
    mixed_check(rng);
  }
  EXPECT(cnf_param_count(nullptr, nullptr) == CNF_ERR_NULL);
  EXPECT(n_ok > iters / 10);
  std::printf("{\"iters\": %d, \"valid_descriptors\": %d, \"failures\": %d}\n", iters, n_ok, g_fail);
  return g_fail ? 1 : 0;
}
