// One-launch Adam step over every parameter of a coupling stack, fed by the
// flat gradient cnf_loss_vjp writes (state_dict order): the on-device
// optimizer of the calibrator's training step (the
// reference steps torch.optim.Adam, calibrators.py:239-295, at its defaults).
//
// Per element, as torch.optim.Adam's single-tensor update (amsgrad off):
//   g  = grad + weight_decay * p
//   m  = m + (1 - beta1) * (g - m)                (exp_avg.lerp_(g, 1 - beta1))
//   v  = beta2 * v + (1 - beta2) * g * g          (exp_avg_sq.mul_().addcmul_())
//   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// The moments live in two flat device buffers the caller owns (cnf_param_count
// floats each, zero before the first step).  The kernel knows only a table of
// tensors and flat offsets: cnf_adam_step_tensors takes that list directly (a
// planar stack's w, u, b), and the cnf_desc entry points derive it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cnf_internal.h"

namespace cnf {
namespace {

constexpr int kAdamTensors = 128;  // parameter tensors per launch (kernel-argument table)

struct AdamArgs {
  float* p[kAdamTensors];
  int64_t off[kAdamTensors + 1];  // flat offset of each tensor, and the end
  const float* g;
  float* m;
  float* v;
  // torch's scalars, each rounded to fp32 once: 1 - beta1 and 1 - beta2 are
  // formed in double from the optimizer's Python floats (torch/optim/adam.py
  // _single_tensor_adam: lerp_(grad, 1 - beta1), addcmul_(value=1 - beta2))
  float omb1, beta2, omb2, eps, wd, step_size, bc2_sqrt;
  // device {step_size, bc2_sqrt} (cnf_adam_step_sched: graph-captured steps,
  // whose kernel arguments are fixed at capture); nullptr: the two above
  const float* sched;
  // device int32 flag (cnf_adam_step_guarded): non-zero skips the whole update,
  // so a step whose gradient tripped the non-finite guard leaves the
  // parameters and moments at the last finite step; nullptr: always update
  const int32_t* skip;
};

__global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
  if (a.skip && __builtin_amdgcn_readfirstlane(*a.skip) != 0) return;
  const int ti = blockIdx.y;
  const int64_t o0 = a.off[ti], n = a.off[ti + 1] - o0;
  float* __restrict__ p = a.p[ti];
  const float step_size = a.sched ? a.sched[0] : a.step_size;
  const float bc2_sqrt = a.sched ? a.sched[1] : a.bc2_sqrt;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t f = o0 + i;
    const float pv = p[i];
    // torch's operation order.  The _rn intrinsics document it and nothing
    // more: in this toolchain they are plain * and +, and under HIP's default
    // contraction the gfx950 code object fuses two of the five multiply-adds
    // into v_fma_f32 (g + wd * p, and p - step_size * (m / denom)); the lerp's
    // product and both of v's are rounded on their own.  Measured against
    // torch.optim.Adam's device steps, this form differs from the single-tensor
    // path in fewer elements than the fully separate one ("Adam
    // sweep").  Division and square root are the correctly rounded sequences,
    // and fp32 subnormals are kept.
    float g = a.g[f];
    if (a.wd != 0.f) g = __fadd_rn(g, __fmul_rn(a.wd, pv));            // grad.add(p, alpha=wd)
    float m = a.m[f];
    m = __fadd_rn(m, __fmul_rn(a.omb1, __fsub_rn(g, m)));              // lerp_(g, 1 - beta1)
    const float v = __fadd_rn(__fmul_rn(a.v[f], a.beta2),
                              __fmul_rn(__fmul_rn(g, g), a.omb2));         // mul_().addcmul_()
    a.m[f] = m;
    a.v[f] = v;
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), a.eps);
    p[i] = __fadd_rn(pv, __fmul_rn(-step_size, __fdiv_rn(m, denom)));    // addcdiv_
  }
}

}  // namespace
}  // namespace cnf

using namespace cnf;

namespace {

// The launches over an explicit tensor list: numel[nt] sizes in flat-gradient
// order.  Every argument is checked before the first launch.
int adam_tensors(int nt, const int64_t* numel, float* const* params, const float* grads,
                 float* exp_avg, float* exp_avg_sq, int64_t step, double lr, double beta1,
                 double beta2, double eps, double weight_decay, const float* sched,
                 const int32_t* skip, void* stream) {
  if (nt < 0) return CNF_ERR_DESC;
  if (!sched && step < 1) return CNF_ERR_DESC;
  if (nt == 0) return CNF_OK;
  if (!numel || !params || !grads || !exp_avg || !exp_avg_sq) return CNF_ERR_NULL;
  for (int i = 0; i < nt; ++i) {
    if (numel[i] < 0) return CNF_ERR_DESC;
    if (!params[i]) return CNF_ERR_NULL;
  }
  const double bc1 = sched ? 1.0 : 1.0 - std::pow(beta1, (double)step);
  const double bc2 = sched ? 1.0 : 1.0 - std::pow(beta2, (double)step);
  AdamArgs a{};
  a.sched = sched;
  a.skip = skip;
  a.g = grads;
  a.m = exp_avg;
  a.v = exp_avg_sq;
  a.omb1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  a.step_size = (float)(lr / bc1);
  a.bc2_sqrt = (float)std::sqrt(bc2);
  int64_t off = 0;
  for (int first = 0; first < nt; first += kAdamTensors) {
    // a chunk's offsets start at its first tensor's flat position
    const int n_here = std::min(kAdamTensors, nt - first);
    int64_t maxn = 0;
    for (int k = 0; k < n_here; ++k) {
      a.p[k] = params[first + k];
      a.off[k] = off;
      off += numel[first + k];
      maxn = std::max(maxn, numel[first + k]);
    }
    a.off[n_here] = off;
    const unsigned gx = (unsigned)std::min<int64_t>((maxn + 255) / 256, 64);
    if (gx == 0) continue;  // every tensor of the chunk is empty
    hipLaunchKernelGGL(k_adam, dim3(gx, (unsigned)n_here), dim3(256), 0, (hipStream_t)stream, a);
  }
  return launch_status();
}

// A coupling stack's tensor sizes in ABI order: per layer, per net, per
// Linear: W then b.
int adam_launch(const cnf_desc* desc, float* const* params, const float* grads, float* exp_avg,
                float* exp_avg_sq, int64_t step, double lr, double beta1, double beta2, double eps,
                double weight_decay, const float* sched, const int32_t* skip, void* stream) {
  Shape s;
  int st = derive_shape(desc, &s);
  if (st != CNF_OK) return st;
  std::vector<int64_t> numel;
  numel.reserve((size_t)s.L * s.nets * s.n_lin * 2);
  for (int l = 0; l < s.L; ++l)
    for (int n = 0; n < s.nets; ++n)
      for (int i = 0; i < s.n_lin; ++i) {
        numel.push_back((int64_t)s.units[i + 1] * s.units[i]);
        numel.push_back(s.units[i + 1]);
      }
  return adam_tensors((int)numel.size(), numel.data(), params, grads, exp_avg, exp_avg_sq, step, lr,
                      beta1, beta2, eps, weight_decay, sched, skip, stream);
}

}  // namespace

extern "C" int cnf_adam_step(const cnf_desc* desc, float* const* params, const float* grads,
                             float* exp_avg, float* exp_avg_sq, int64_t step, double lr,
                             double beta1, double beta2, double eps, double weight_decay,
                             void* stream) {
  CNF_RANGE("cnf_adam_step");
  return adam_launch(desc, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
                     weight_decay, nullptr, nullptr, stream);
}

extern "C" int cnf_adam_step_sched(const cnf_desc* desc, float* const* params,
                                   const float* grads, float* exp_avg, float* exp_avg_sq,
                                   const float* sched, double beta1, double beta2, double eps,
                                   double weight_decay, void* stream) {
  CNF_RANGE("cnf_adam_step_sched");
  if (!sched) return CNF_ERR_NULL;
  return adam_launch(desc, params, grads, exp_avg, exp_avg_sq, 0, 0.0, beta1, beta2, eps,
                     weight_decay, sched, nullptr, stream);
}

extern "C" int cnf_adam_step_guarded(const cnf_desc* desc, float* const* params,
                                     const float* grads, float* exp_avg, float* exp_avg_sq,
                                     int64_t step, double lr, const float* sched, double beta1,
                                     double beta2, double eps, double weight_decay,
                                     const int32_t* skip_flag, void* stream) {
  CNF_RANGE("cnf_adam_step_guarded");
  if (!skip_flag) return CNF_ERR_NULL;
  return adam_launch(desc, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps,
                     weight_decay, sched, skip_flag, stream);
}

extern "C" int cnf_adam_step_tensors(int32_t n_tensors, const int64_t* numel, float* const* params,
                                     const float* grads, float* exp_avg, float* exp_avg_sq,
                                     int64_t step, double lr, const float* sched, double beta1,
                                     double beta2, double eps, double weight_decay,
                                     const int32_t* skip_flag, void* stream) {
  CNF_RANGE("cnf_adam_step_tensors");
  return adam_tensors(n_tensors, numel, params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2,
                      eps, weight_decay, sched, skip_flag, stream);
}
