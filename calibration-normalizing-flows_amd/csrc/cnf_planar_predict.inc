// The body of cnf_planar.hip's k_planar_predict and k_planar_score, included
// once in each.  CNF_SCORE 0 (k_planar_predict): the token stream is the
// kernel's body as it was before the score variant existed, so its code is
// unchanged.  CNF_SCORE 1 (k_planar_score): the scoring epilogue of
// cnf_score.h takes the fp32 probabilities in place of the store; there is no
// store phase and the log-det is not written.
//
// Names the including kernel provides: x, blob, lp, D, L, cs, B (both);
// probs, ld_out (predict); sc, the kernel's score::Args, and rec, its
// __shared__ long long[score::kRecWords] record (score).
//
// Why an include and not one `template <bool SCORE>` device function with
// `if constexpr`: that form was tried and tools/isa_diff.py showed all 22
// k_planar_predict instantiations changing (register allocation and
// instruction order, e.g. <1,10> 1658 -> 1655 lines), and the score variant
// must leave predict's code as it is.
  constexpr int RPB = kThreads / LPR;
#if CNF_SCORE
  score::Acc acc;
  score::init(rec, sc.bins);
#endif
  constexpr bool kStage = LPR == 1;
  constexpr int TS = CPL | 1;
  __shared__ float tile[kStage ? kThreads * TS : 1];
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
    for (int l = 0; l < L; ++l) planar_step<LPR, CPL>(xv, blob + (size_t)l * cs, gl, ld);
#if !CNF_SCORE
    if (valid && ld_out && gl == 0) ld_out[row] = ld;
#endif
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
#if CNF_SCORE
    score::row<LPR, CPL>(xv, gl, D, valid ? sc.y[row] : -1, valid, sc.bins, sc.e, rec, acc);
#else
    if constexpr (kStage) {
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
#endif
  }
#if CNF_SCORE
  score::flush(rec, sc.bins, acc, sc.record);
#endif
