/*
 * cnf.h -- C ABI of libcnf_hip.so, the MI355X (gfx950) coupling-flow engine.
 *
 * Drop-in native boundary for the RealNVP / NICE forward, inverse and
 * log|det J| path of the reference (SergioAlvarezB/calibration-normalizing-flows):
 *
 *   cnf_forward   replaces Flow.forward            flows/flows.py:17-25
 *                 (NvpCouplingLayer.forward         flows/flows.py:101-112,
 *                  MLP.forward                      flows/utils.py:26-31)
 *   cnf_inverse   replaces Flow.backward           flows/flows.py:27-37
 *                 (NvpCouplingLayer.backward        flows/flows.py:114-126 -- the
 *                  reference's "backward" is the INVERSE transform, not autograd)
 *   cnf_prepare   replaces the per-layer parameter reads of the above
 *                 (state_dict layout: flows/flows.py:76-99, flows/utils.py:14-22)
 *   cnf_loss_vjp  replaces autograd of the calibrator loss
 *                 calibrators.py:287-295 / run_experiment3D.py:102-107
 *
 * Plain C: pointers + sizes, no torch types.  Every device pointer is a HIP
 * device allocation owned by the caller; all work is enqueued on the caller's
 * stream (hipStream_t passed as void*), nothing synchronises the host, nothing
 * allocates, so every entry point is graph-capturable (cnf_prepare included
 * once its host tables are built -- see below).  Errors are returned as
 * negative cnf_status codes; no exception crosses the ABI.
 *
 * Data layout: row-major fp32 logit batches [B][D] (one logit vector per row).
 */
#ifndef CNF_H_
#define CNF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNF_ABI_VERSION 2   /* 2: cnf_adam_step takes double hyper-parameters */
#define CNF_MAX_HIDDEN 8    /* hidden layers per conditioner MLP            */
#define CNF_MAX_DIM 256     /* logit-vector width D                         */
#define CNF_MAX_WIDTH 512   /* any MLP width                                */

typedef enum cnf_status {
  CNF_OK = 0,
  CNF_ERR_NULL = -1,          /* a required pointer is NULL                   */
  CNF_ERR_DESC = -2,          /* malformed descriptor (dims, abi_version)     */
  CNF_ERR_UNSUPPORTED = -3,   /* shape outside every kernel's envelope        */
  CNF_ERR_BATCH = -4,         /* negative batch, or above cnf_metrics' row limit */
  CNF_ERR_HIP = -5,           /* a HIP launch/copy failed (cnf_last_hip_error) */
  CNF_ERR_ALIGN = -6          /* pointer not aligned to its element (4 or 8 bytes) */
} cnf_status;

/* The shape of one Flow made of NvpCouplingLayers (flows/flows.py:68-99). */
typedef struct cnf_desc {
  int32_t abi_version;          /* = CNF_ABI_VERSION                              */
  int32_t dim;                  /* D (n_classes), 2..CNF_MAX_DIM                  */
  int32_t n_layers;             /* L >= 1                                         */
  int32_t n_hidden;             /* len(hidden_size), 0..CNF_MAX_HIDDEN            */
  int32_t hidden[CNF_MAX_HIDDEN];
  int32_t scale;                /* 1: s-net present (RealNVP); 0: NICE, s == 0    */
  int32_t shift;                /* 1: t-net present; 0: t == 0                    */
  int32_t strict_nan;           /* 1: reproduce the reference's inf*0 = NaN at
                                   masked positions (flows/flows.py:107,123)      */
  int32_t options;              /* CNF_OPT_* bits (0: pick the fastest kernel)    */
  const int64_t* perms;         /* HOST pointer, NULL or L*D entries: layer l's
                                   random_flip permutation (flows/flows.py:92-99);
                                   a row whose first entry is < 0 = no perm      */
} cnf_desc;

/* cnf_desc.options: keep a launch off a kernel family (A/B and test use;
 * results agree to fp32 rounding either way). */
#define CNF_OPT_NO_SGPR 1   /* narrow flows: k_valu instead of k_sgpr          */
#define CNF_OPT_NO_WIDE 2   /* wide flows: k_tile instead of k_wide            */
/* Legacy semantics of the reference's TensorFlow flows (code-old/realNVP.py:
 * 19-92; parity unpinned -- TensorFlow is absent):
 *   ALT_MASK  the coupling mask alternates per layer (layer l transforms the
 *             first D//2 features when l is even, the last D//2 when l is
 *             odd) and the data are never flipped (code-old/realNVP.py:66-76);
 *             parameters keep the layer's own column / row order;
 *   S_TANH    the s-net's hidden activations are tanh (code-old/realNVP.py:
 *             58-64); the t-net keeps ReLU.
 * Forward / inverse: k_valu for the narrow shapes of its tables (the code-old
 * default hidden=[dim] at D=3 and 10, and [5,5]), the MFMA-tile family for
 * every other shape; reverse mode: the layer-at-a-time kernels of
 * cnf_wvjp.hip.  Not combinable with random_flip permutations or strict_nan. */
#define CNF_OPT_ALT_MASK 4
#define CNF_OPT_S_TANH 8

/* One float per parameter, in the reference's state_dict order. */
int cnf_param_count(const cnf_desc* desc, int64_t* n_floats);

/* Number of parameter tensors cnf_prepare expects, in this order per layer
 * l = 0..L-1:  [s.layers.0.weight, s.layers.0.bias, ..., s.layers.k.bias]
 * (if scale), then the same for t (if shift).  Weight [out][in] row-major. */
int cnf_param_tensor_count(const cnf_desc* desc, int32_t* n_tensors);

/* Bytes of the device blob cnf_prepare writes (kernel-specific layout). */
int cnf_prepared_bytes(const cnf_desc* desc, size_t* bytes);

/* Reformat the parameters into the blob the selected kernel reads: the mask,
 * the per-layer flip and any random_flip permutation are folded into index
 * tables; weights are restricted to the unmasked block and tiled for the
 * kernel.  params: HOST array of cnf_param_tensor_count DEVICE pointers. */
int cnf_prepare(const cnf_desc* desc, const float* const* params, void* prepared,
                void* stream);

/* Forward + per-sample log-det (Flow.forward):
 *   x      [B][D]      input logits
 *   z      [B][D]      final output (= zs[-1]); may be NULL when z_all != NULL
 *   logdet [B]         sum over layers of sum_j (1-mask_j) s_j; may be NULL
 *   z_all  [L][B][D]   every layer's output (the reference's zs list); may be NULL */
int cnf_forward(const cnf_desc* desc, const void* prepared, const float* x, float* z,
                float* logdet, float* z_all, int64_t B, void* stream);

/* Inverse + log-det (Flow.backward): layers applied L-1..0.
 *   x_all  [L][B][D]   xs list in the reference's order (x_all[L-1] = input
 *                       estimate); may be NULL.  logdet = -(forward log-det). */
int cnf_inverse(const cnf_desc* desc, const void* prepared, const float* z, float* x,
                float* logdet, float* x_all, int64_t B, void* stream);

/* Loss kinds for cnf_forward_loss / cnf_loss_vjp. */
#define CNF_LOSS_CAL 0  /* -mean(log(softmax(z_L)[y] + 1e-7) + ld)   calibrators.py:287-291 */
#define CNF_LOSS_CE 1   /* CE(z_L, y) - det * mean(ld)               run_experiment3D.py:107 */

/* Fused forward + log-det + loss terms (the eval pass of TorchFlowCalibrator.fit,
 * calibrators.py:297-317; the per-step NLL of a sharded batch):
 *   loss_terms[3]  {sum of per-row loss, sum of ce, sum of ld} over the B rows
 *   z, logdet      as cnf_forward, each may be NULL
 * The fused pass writes per-block partial sums into the workspace (no
 * initialisation needed); a one-block follow-up launch adds them in block
 * order (deterministic).  Narrow flows only (sgpr-fused / valu-fused). */
int cnf_forward_loss_workspace_bytes(const cnf_desc* desc, int64_t B, size_t* bytes);
int cnf_forward_loss(const cnf_desc* desc, const void* prepared, const float* x,
                     const int64_t* y, int32_t loss_kind, float det, float* z, float* logdet,
                     float* loss_terms, int64_t B, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Fused calibrated prediction: Calibrator.predict of the flow calibrator
 * (calibrators.py:40-44 with TorchFlowCalibrator.predict_post, :330-353), per row
 *   p = softmax(flow(x - mean(x))),  probs = softmax(log(p + 1e-7) - log_priors)
 *   log_priors [D]     DEVICE pointer (the calibrator's log class priors)
 *   probs      [B][D]  calibrated probabilities
 *   logdet     [B]     log-det of the centred rows, may be NULL
 * Served by k_sgpr (the narrow shapes, random_flip included) and k_wide (the
 * wide shapes of its table, e.g. D=100, hidden [100,100]); CNF_ERR_UNSUPPORTED
 * otherwise (strict_nan, legacy options, other wide shapes: the caller then
 * composes cnf_forward with its own softmax). */
int cnf_predict(const cnf_desc* desc, const void* prepared, const float* x,
                const float* log_priors, float* probs, float* logdet, int64_t B, void* stream);

/* Workspace bytes cnf_vjp / cnf_loss_vjp need for a batch of B rows. */
int cnf_vjp_workspace_bytes(const cnf_desc* desc, int64_t B, size_t* bytes);

/* Reverse mode of cnf_forward (the autograd backward of Flow.forward):
 * given upstream gradients of its outputs, writes
 *   grads  [cnf_param_count]  d/d(parameters), state_dict order (overwritten)
 *   dx     [B][D]             d/dx, may be NULL
 * Upstream inputs, each may be NULL (= zero):
 *   gz     [B][D]     gradient of the final z
 *   gz_all [L][B][D]  gradient of every layer output (the zs list)
 *   gld    [B]        gradient of the per-sample log-det
 * The forward pass is recomputed inside (nothing is saved between calls). */
int cnf_vjp(const cnf_desc* desc, const void* prepared, const float* x, const float* gz,
            const float* gz_all, const float* gld, float* grads, float* dx, int64_t B,
            void* workspace, size_t workspace_bytes, void* stream);

/* Fused forward + loss + reverse mode.  Writes
 *   loss_terms[3]   {sum over rows of the per-row loss, sum of ce, sum of ld}
 *                   (divide by the GLOBAL batch to get the reference's means;
 *                   the split lets data-parallel ranks all-reduce sums)
 *   grads           gradient of (sum over THIS batch of the per-row loss) *
 *                   grad_scale, in cnf_param_count / state_dict order.
 *                   Overwritten, not accumulated.
 *   dx [B][D]       d(loss)/dx, may be NULL
 * Deterministic: no float atomics; fixed-order reductions. */
int cnf_loss_vjp(const cnf_desc* desc, const void* prepared, const float* x,
                 const int64_t* y, int32_t loss_kind, float det, float grad_scale,
                 float* loss_terms, float* grads, float* dx, int64_t B, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Reverse mode of cnf_inverse (autograd through Flow.backward, flows/flows.py:
 * 27-37 / 114-126): given upstream gradients of the inverse's outputs, writes
 *   grads  [cnf_param_count]  d/d(parameters), state_dict order (overwritten)
 *   dz     [B][D]             d/dz, may be NULL
 * Upstream inputs, each may be NULL (= zero):
 *   gx     [B][D]     gradient of the final output (xs[-1], the input estimate)
 *   gx_all [L][B][D]  gradient of every step's output (the xs list, step order)
 *   gld    [B]        gradient of the inverse's per-sample log-det
 * Layer-at-a-time MFMA reverse mode for every shape; strict_nan follows
 * torch autograd's rules for the reference's op sequence (NaN / inf kept). */
int cnf_vjp_inverse_workspace_bytes(const cnf_desc* desc, int64_t B, size_t* bytes);
int cnf_vjp_inverse(const cnf_desc* desc, const void* prepared, const float* z, const float* gx,
                    const float* gx_all, const float* gld, float* grads, float* dz, int64_t B,
                    void* workspace, size_t workspace_bytes, void* stream);

/* One Adam step over every parameter (torch.optim.Adam's update, amsgrad off;
 * the optimizer of TorchFlowCalibrator.fit, calibrators.py:239-295) in one
 * launch, fed by the flat gradient of cnf_loss_vjp / cnf_vjp:
 *   params      HOST array of cnf_param_tensor_count DEVICE pointers, updated
 *               in place (the tensors cnf_prepare reads)
 *   grads       [cnf_param_count]  flat, state_dict order
 *   exp_avg, exp_avg_sq  [cnf_param_count] moments, zero before step 1
 *   step        1-based step count (bias corrections)
 *   lr, beta1, beta2, eps, weight_decay   as the torch optimizer holds them
 *               (Python floats = doubles): 1 - beta, the bias corrections and
 *               lr / (1 - beta1^t) are formed in double and rounded to fp32
 *               once, as torch's scalar arguments are */
int cnf_adam_step(const cnf_desc* desc, float* const* params, const float* grads,
                  float* exp_avg, float* exp_avg_sq, int64_t step, double lr, double beta1,
                  double beta2, double eps, double weight_decay, void* stream);

/* The same step with its two step-dependent scalars read from DEVICE memory,
 * so a HIP graph captured once replays any step (kernel arguments are fixed at
 * capture):  sched[0] = (float)(lr / (1 - beta1^t)),
 *            sched[1] = (float)sqrt(1 - beta2^t)   (formed in double). */
int cnf_adam_step_sched(const cnf_desc* desc, float* const* params, const float* grads,
                        float* exp_avg, float* exp_avg_sq, const float* sched, double beta1,
                        double beta2, double eps, double weight_decay, void* stream);

/* cnf_adam_step (sched == NULL: step and lr as there) or cnf_adam_step_sched
 * (sched != NULL: step and lr ignored) that first reads the DEVICE int32
 * *skip_flag -- the flag cnf_guard_nonfinite ORs into -- and, when it is
 * non-zero, updates nothing: the parameters and both moments keep the last
 * finite step's values, as the reference keeps its weights when it breaks out
 * of the loop before opt.step() on NaN (run_experiment3D.py:129-133).  No host
 * sync: the guard's scan of the gradient and this step queue on one stream. */
int cnf_adam_step_guarded(const cnf_desc* desc, float* const* params, const float* grads,
                          float* exp_avg, float* exp_avg_sq, int64_t step, double lr,
                          const float* sched, double beta1, double beta2, double eps,
                          double weight_decay, const int32_t* skip_flag, void* stream);

/* The same kernel over an explicit tensor list, for parameters that no cnf_desc
 * describes (a planar stack's w, u, b):
 *   n_tensors   tensors in the list (0: nothing to do)
 *   numel       HOST array of n_tensors sizes, in flat-gradient order: tensor i
 *               owns grads / exp_avg / exp_avg_sq [sum numel[<i], + numel[i])
 *   params      HOST array of n_tensors DEVICE pointers, updated in place
 *   sched       NULL: (step, lr) as cnf_adam_step; else the DEVICE
 *               {step_size, bc2_sqrt} of cnf_adam_step_sched (step, lr ignored)
 *   skip_flag   NULL, or the DEVICE int32 flag of cnf_adam_step_guarded
 * n_tensors < 0, numel < 0, or step < 1 without sched: CNF_ERR_DESC; a NULL
 * table entry: CNF_ERR_NULL -- all before any launch.  More than 128 tensors
 * go out as one launch per 128. */
int cnf_adam_step_tensors(int32_t n_tensors, const int64_t* numel, float* const* params,
                          const float* grads, float* exp_avg, float* exp_avg_sq,
                          int64_t step, double lr, const float* sched, double beta1,
                          double beta2, double eps, double weight_decay,
                          const int32_t* skip_flag, void* stream);

/* Device-side non-finite guard (failure detection; the counterpart of the
 * reference's NaN abort, run_experiment3D.py:129-131, without a host sync):
 * scans n floats of a DEVICE array (z, logdet, loss_terms, gradients ...) and
 * ORs into the caller-owned DEVICE int32 *flag:  1 if any element is NaN,
 * 2 if any is +-inf.  The flag is never cleared by the library, so one
 * zeroed flag can accumulate over many launches and be read once.  One
 * HBM-bound pass; an atomic OR only from a wave that found something. */
int cnf_guard_nonfinite(const float* data, int64_t n, int32_t* flag, void* stream);

/* On-device calibration scoring of a probability matrix (the reference's
 * utils/metrics.py:6-15, 35-80: neg_log_likelihood, expected_calibration_error,
 * accuracy), e.g. of cnf_predict's output, without copying it to the host:
 *   probs  [B][D]  fp32 probabilities, 2 <= D <= CNF_MAX_DIM
 *   y      [B]     int64 labels
 *   bins           1..CNF_MAX_BINS equal-width confidence bins (reference: 15)
 * Per row the prediction is the FIRST index of the row maximum (np.argmax),
 * the confidence is that maximum, and bin i holds the row iff
 * i*width < conf <= (i+1)*width, conf widened to double, width = 1.0/bins in
 * double (a confidence <= 0 or > 1 falls in no bin).  The NLL term is
 * -log(p[y] + 1e-7) on the widened p[y].  A row whose label is outside
 * [0, D), that holds a non-finite entry, or whose p[y] + 1e-7 is not positive
 * (no finite term) counts in n_invalid and in nothing else. */
#define CNF_MAX_BINS 64
/* record: int64 words
 *   [0] n_rows   [1] n_invalid   [2] nll_fx   [3] n_correct
 *   [4 .. 4+bins)          rows per bin
 *   [4+bins .. 4+2*bins)   conf_fx per bin
 *   [4+2*bins .. 4+3*bins) correct rows per bin
 * *_fx: sums of rint(value * 2^32), value widened to double first
 * n_rows counts the valid rows.  Every word is an integer sum, so a record is
 * bitwise repeatable and independent of grid, batch split and shard split;
 * records of shards add word by word.  cnf_metrics ADDS into `record`: the
 * caller zeroes it once (as with cnf_guard_nonfinite's flag), so one record
 * can cover many batches or graph replays.  A term is < 2^5, so one record
 * holds 2^26 rows; B > 2^26 is CNF_ERR_BATCH.  The workspace size is 0 (blocks
 * add with integer atomics; workspace may be NULL). */
int cnf_metrics_record_words(int32_t bins, int64_t* words);
int cnf_metrics_workspace_bytes(int32_t dim, int32_t bins, int64_t B, size_t* bytes);
int cnf_metrics(const float* probs, const int64_t* y, int32_t dim, int32_t bins, int64_t B,
                int64_t* record, void* workspace, size_t workspace_bytes, void* stream);

/* Temperature, MLR, vector and matrix scaling on the device: the objective and
 * gradient sums that the reference's fits hand to SciPy (TempScalingCalibrator,
 * MatrixScalingCalibrator, VectorScalingCalibrator, MLRCalibrator,
 * calibrators.py:57-205; optim_temperature, utils/ops.py:69-115) and the
 * calibrated prediction of the fitted map, for logits resident on the device.
 * All four minimise mean(-log(softmax(t)[y] + 1e-7)) over an affine map of
 * the logits:
 *   CNF_SCALE_SCALAR  t = a*x + b    a: 1 double; b: D doubles or NULL (= 0)
 *                     (temperature scaling: a = 1/T, no bias; MLR)
 *   CNF_SCALE_DIAG    t = w.x + b    a = w: D doubles; b: D   (vector scaling)
 *   CNF_SCALE_FULL    t = x@W + b    a = W: [D][D] row-major, input x output,
 *                     as the reference's `logits @ W`; b: D   (matrix scaling)
 * x is fp32 [B][D]; a, b, log_priors and sums are DEVICE float64 arrays.  The
 * logits are widened on load and everything after that -- the map, the row
 * maximum, exp, the sum, log, the gradient terms, the sums over rows -- is
 * float64 (SciPy's Newton-CG differences the gradient below an fp32 ulp of T).
 * Scalar and diagonal kinds: 2 <= D <= CNF_MAX_DIM; full kind: 2 <= D <= 128
 * (CNF_ERR_UNSUPPORTED above).  B <= 2^26 (CNF_ERR_BATCH above). */
#define CNF_SCALE_SCALAR 0
#define CNF_SCALE_DIAG 1
#define CNF_SCALE_FULL 2

/* Words of `sums` with want_grad: 1 + D + (1 | D | D*D by kind). */
int cnf_scaling_sums_words(int32_t kind, int32_t dim, int64_t* words);
/* Bytes of per-block float64 partial sums a call of B rows writes. */
int cnf_scaling_workspace_bytes(int32_t kind, int32_t dim, int64_t B, size_t* bytes);

/* One fused pass over (x, y [B] int64 labels).  With p_r = softmax(t_r)
 * (row maximum subtracted first, as SciPy's softmax) and g_r = p_r - onehot(y_r):
 *   sums[0]          sum_r -log(p_r[y_r] + 1e-7)
 * and, when want_grad != 0,
 *   sums[1 .. 1+D)   sum_r g_rj
 *   then `ga`:       scalar kind  1 word   sum_r sum_j g_rj x_rj
 *                    diagonal     D words  sum_r g_rj x_rj
 *                    full         D*D      ga[i*D + j] = sum_r x_ri g_rj
 * Raw sums: the caller divides by B and forms the reference's formulas.  With
 * want_grad == 0 only sums[0] is written.  A label outside [0, D) turns
 * sums[0] and every gradient word into NaN.  B == 0 zeroes the words and
 * launches no kernel.  Deterministic: per-block partials in `workspace`, added
 * in block order by a follow-up launch; the grid depends on (kind, D, B) only,
 * so two calls agree bitwise.  No float atomics, no allocation, no host sync. */
int cnf_scaling_loss_grad(const float* x, const int64_t* y, int32_t kind, int32_t dim,
                          const double* a, const double* b, int32_t want_grad, int64_t B,
                          double* sums, void* workspace, size_t workspace_bytes, void* stream);

/* Fused Calibrator.predict of a scaling map (calibrators.py:40-44 with the
 * predict_post of :67, :113, :158, :202), per row
 *   p = softmax(t(x - mean(x))),  probs = softmax(log(p + 1e-7) - log_priors)
 * computed in float64 and rounded once into fp32 probs [B][D] (ready for
 * cnf_metrics).  log_priors: D DEVICE doubles.  Same envelope as above. */
int cnf_scaling_predict(const float* x, int32_t kind, int32_t dim, const double* a,
                        const double* b, const double* log_priors, float* probs, int64_t B,
                        void* stream);

/* Isotonic (pool-adjacent-violators) calibration, the reference's PAVCalibrator
 * (calibrators.py:208-236): one sklearn IsotonicRegression(y_min=0, y_max=1,
 * out_of_bounds='clip') per class on softmax(centred logits)[:, c].  The fit
 * runs on the host (cnf_hip/pav.py); the device serves the prediction.
 * 2 <= D <= CNF_MAX_DIM; B <= 2^26 (CNF_ERR_BATCH above).
 *
 * The model of class c is n_thr[c] points (thr_x[c][k], thr_y[c][k]), thr_x
 * strictly increasing, thr_y non-decreasing (sklearn's X_thresholds_ /
 * y_thresholds_), in arrays thr_x, thr_y [D][cap] of doubles, cap >= 1
 * (CNF_ERR_DESC otherwise), and n_thr [D] of int32, all DEVICE memory. */

/* Fused PAVCalibrator.predict (calibrators.py:40-44, 228-236), one launch: per
 * row s = softmax(x - mean(x)) in float64; per class s_c clipped to
 * [thr_x[c][0], thr_x[c][n-1]] and interpolated linearly between the points
 * (SciPy interp1d's rule; n = min(n_thr[c], cap); n == 1 is the constant
 * thr_y[c][0], n == 0 gives 0); each row divided by its sum (a row of zeros
 * becomes NaN, as in the reference); probs = softmax(log(p + 1e-7) -
 * log_priors), rounded once into fp32 probs [B][D] (ready for cnf_metrics).
 * log_priors: D DEVICE doubles.  The tables are staged in LDS when
 * D * cap <= 2048 and searched in global memory otherwise.  Enqueued on
 * `stream`; no allocation, no host synchronisation; B == 0 launches nothing. */
int cnf_pav_predict(const float* x, int32_t dim, int64_t B, const double* thr_x,
                    const double* thr_y, const int32_t* n_thr, int32_t cap,
                    const double* log_priors, float* probs, void* stream);

/* Planar flows: a Flow of the reference's PlanarLayers (flows/flows.py:129-165;
 * get_Planarmodel / train_planar of the calibration notebooks).  Per layer,
 * with parameters w [D], u [D], b [1] (that state_dict order):
 *   wtu = w.u,  m = -1 + log1p(exp(wtu)),  u_hat = u + ((m - wtu) * w) / ||w||
 *   h = tanh(x.w + b),  z = x + h * u_hat,  log_det = log|1 + (1 - h^2) (w.u_hat)|
 * (the division is by the norm, not its square, and ||w|| = 0 gives NaN, as in
 * the reference; the log-det is -inf where its argument is 0).  All fp32.
 *   dim       D, 1..CNF_MAX_DIM;  n_layers  L, 1..CNF_PLANAR_MAX_LAYERS
 *             (< 1: CNF_ERR_DESC; above: CNF_ERR_UNSUPPORTED)
 *   params    HOST array of 3 * L DEVICE pointers: w, u, b of layer 0, 1, ...
 *   B         0..2^31 rows (CNF_ERR_BATCH otherwise)
 *   workspace cnf_planar_workspace_bytes(dim, n_layers, B) bytes of DEVICE
 *             memory, no initialisation needed; one size serves every entry
 *             point.  A call first writes each layer's (w, u_hat, b, w.u_hat)
 *             there with one small launch, which every kernel of the call
 *             reads, so nothing is cached between calls.
 * In floats, with LPR = 1 (D <= 16), 16 (D <= 64) or 64 lanes per row,
 * DP = D rounded up to a multiple of LPR, PW = L * (2 D + 2) + 4 and r64(n) = n
 * rounded up to a multiple of 64, the workspace holds
 *   r64(L * (2 DP + 8)) + r64(PW) + r64(max(U * PW, 4 * F)) + (L > 10 ? r64(L * B) : 0)
 * where F = min(1024, ceil(B * LPR / 256)) blocks of the forward grid (at
 * least 1) and U the records of the reverse grid: C = min(256, ceil(B * LPR /
 * 256)) blocks when PW <= 3072, else 4 records for each of min(C, max(4,
 * 2^20 / PW)) blocks.  The last term is the per-(row, layer) tanh tape of
 * stacks deeper than 10 layers (shallower ones keep it in registers).
 * Argument errors (NULL, alignment, shape, batch) are returned before any
 * launch; B == 0 zeroes loss_terms / grads with memset nodes and launches no
 * kernel.  Deterministic: per-block partial sums added in block order by a
 * one-block follow-up launch; the grids depend on (D, L, B) only, so two calls
 * agree bitwise.  No float atomics, no allocation, no host synchronisation. */
#define CNF_PLANAR_MAX_LAYERS 64

/* 3 * L tensors, L * (2 D + 1) floats. */
int cnf_planar_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats);
int cnf_planar_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B, size_t* bytes);
/* What a call of this shape launches (host only, no launch; argument errors as
 * cnf_planar_workspace_bytes), computed by the functions the launches use:
 *   out = {LPR, CPL (columns per lane, DP / LPR), regt, rega, gacc,
 *          forward blocks F, reverse blocks, reverse records U}
 * regt: the reverse mode keeps its tape in registers (L <= 10); rega: and its
 * row sums in per-lane accumulators (LPR == 1, D <= 11); gacc: the wave
 * records live in the workspace (PW > 3072).  The forward, predict and score
 * kernels are the <LPR, CPL> instantiation, the reverse kernel <LPR, CPL, regt,
 * rega>.  The block counts at B == 0 are those of B == 1 (no kernel runs). */
int cnf_planar_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]);

/* Flow.forward of the stack: z [B][D] (= zs[-1]), logdet [B] (the sum over
 * layers), z_all [L][B][D] (the zs list); each may be NULL. */
int cnf_planar_forward(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, float* z, float* logdet, float* z_all, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Forward + loss terms, as cnf_forward_loss: loss_terms[3] = {sum of per-row
 * loss, sum of ce, sum of ld} for CNF_LOSS_CAL / CNF_LOSS_CE; z, logdet may be
 * NULL.  A label outside [0, D) makes the terms NaN. */
int cnf_planar_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                            const float* x, const int64_t* y, int32_t loss_kind, float det,
                            float* z, float* logdet, float* loss_terms, int64_t B,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Calibrator.predict of a planar flow calibrator, per row:
 *   xc = x - mean(x);  z = planar stack(xc);  p = softmax(z)
 *   probs = softmax(log(p + 1e-7) - log_priors)
 * in one pass that keeps the row in registers.  log_priors [D] DEVICE floats
 * (as cnf_predict; a -inf entry makes every row NaN, as the reference's is);
 * probs [B][D]; logdet [B] of the centred rows, may be NULL.  Same envelope,
 * workspace function, prepare launch, argument validation, B == 0 rule and
 * determinism as cnf_planar_forward. */
int cnf_planar_predict(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, const float* log_priors, float* probs, float* logdet,
                       int64_t B, void* workspace, size_t workspace_bytes, void* stream);
/* The score variant of cnf_planar_predict: ONE launch that runs the predict
 * arithmetic up to the fp32 probability it would store and, instead of storing
 * it, ADDS the row into `record` exactly as cnf_metrics would from the stored
 * matrix -- the record layout, validity rules, bin thresholds and add-into
 * contract documented at cnf_metrics -- so
 *   cnf_planar_score(x, ..., y, bins, record)
 * leaves the words of cnf_planar_predict(x, ..., probs) followed by
 * cnf_metrics(probs, y, ...) without the [B][D] matrix going to memory (the
 * log-det is not produced).  y: [B] int64 DEVICE labels.  Grid, rows per
 * block, workspace and prepare launch are the sibling's.  Validation is the
 * sibling's plus cnf_metrics': 2 <= dim, bins in 1..CNF_MAX_BINS
 * (CNF_ERR_DESC), B <= 2^26 (CNF_ERR_BATCH), y and record 8-byte aligned
 * (CNF_ERR_ALIGN), record non-NULL; all before any HIP call.  B == 0 returns
 * CNF_OK without a launch and leaves the record as it is. */
int cnf_planar_score(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                     const float* log_priors, const int64_t* y, int32_t bins, int64_t* record,
                     int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Reverse mode of cnf_planar_forward, as cnf_vjp: upstream gz [B][D], gz_all
 * [L][B][D], gld [B] (each may be NULL = zero); writes grads
 * [cnf_planar_param_count] (per layer w, u, b; overwritten) and dx [B][D]
 * (may be NULL).  The forward pass is recomputed inside; the only tape is one
 * tanh value per (row, layer). */
int cnf_planar_vjp(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                   const float* gz, const float* gz_all, const float* gld, float* grads,
                   float* dx, int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Fused forward + loss + reverse mode, as cnf_loss_vjp: loss_terms[3] (sums
 * over this batch), grads = grad_scale * d(sum of the per-row loss)/d(params),
 * dx [B][D] = grad_scale * d(sum of the per-row loss)/dx, may be NULL. */
int cnf_planar_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                        const float* x, const int64_t* y, int32_t loss_kind, float det,
                        float grad_scale, float* loss_terms, float* grads, float* dx, int64_t B,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Radial flows: a Flow of the reference's RadialLayers (flows/flows.py:168-193;
 * the radial calibrator of the calibration notebooks).  Per layer, with
 * parameters z0 [D], a [1], b [1] (that state_dict order):
 *   sp = log1p(exp(b)),  beta = -a + sp
 *   d = x - z0,  r = ||d||_2,  h = 1 / (a + r),  z = x + beta * h * d
 * The layer's log-det is the reference's constant log(1.0) = 0 (a quirk, kept):
 * no entry point takes or produces a log-det, and the third loss term is 0.
 * IEEE division and square root; a + r == 0 gives h = inf and a row with
 * r == 0 there becomes NaN, as in the reference.  All fp32.
 *   dim       D, 1..CNF_MAX_DIM;  n_layers  L, 1..CNF_RADIAL_MAX_LAYERS
 *             (< 1: CNF_ERR_DESC; above: CNF_ERR_UNSUPPORTED)
 *   params    HOST array of 3 * L DEVICE pointers: z0, a, b of layer 0, 1, ...
 *   B         0..2^31 rows (CNF_ERR_BATCH otherwise)
 *   workspace cnf_radial_workspace_bytes(dim, n_layers, B) bytes of DEVICE
 *             memory, no initialisation needed; one size serves every entry
 *             point.  A call first writes each layer's (z0, a, sp, beta,
 *             sigmoid(b)) there with one small launch, which every kernel of
 *             the call reads, so nothing is cached between calls.
 * In floats, with LPR = 1 (D <= 16), 16 (D <= 64) or 64 lanes per row,
 * DP = D rounded up to a multiple of LPR, PW = L * (D + 2) + 4 and r64(n) = n
 * rounded up to a multiple of 64, the workspace holds
 *   r64(L * (DP + 8)) + r64(PW) + r64(max(U * PW, 4 * F)) + (L > 10 ? r64(L * B) : 0)
 * where F = min(1024, ceil(B * LPR / 256)) blocks of the forward grid (at
 * least 1) and U the records of the reverse grid: C = min(256, ceil(B * LPR /
 * 256)) blocks when PW <= 3072, else 4 records for each of min(C, max(4,
 * 2^20 / PW)) blocks.  The last term is the per-(row, layer) tape of r for
 * stacks deeper than 10 layers (shallower ones keep it in registers).
 * Argument errors (NULL, alignment, shape, batch) are returned before any
 * launch; B == 0 zeroes loss_terms / grads with memset nodes and launches no
 * kernel.  Deterministic: per-block partial sums added in block order by a
 * one-block follow-up launch; the grids depend on (D, L, B) only, so two calls
 * agree bitwise.  No float atomics, no allocation, no host synchronisation. */
#define CNF_RADIAL_MAX_LAYERS 64

/* 3 * L tensors, L * (D + 2) floats. */
int cnf_radial_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats);
int cnf_radial_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B, size_t* bytes);
/* As cnf_planar_launch_plan; rega: LPR == 1 at L <= 10, whatever the width. */
int cnf_radial_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]);

/* Flow.forward of the stack: z [B][D] (= zs[-1]) and z_all [L][B][D] (the zs
 * list); each may be NULL. */
int cnf_radial_forward(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, float* z, float* z_all, int64_t B, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Forward + loss terms: loss_terms[3] = {sum of per-row loss, sum of ce, 0}
 * for CNF_LOSS_CAL (ce = -log(softmax(z)[y] + 1e-7)) / CNF_LOSS_CE
 * (ce = -log softmax(z)[y]); the log-det being 0, loss == ce and there is no
 * `det` weight.  z may be NULL.  A label outside [0, D) makes the terms NaN. */
int cnf_radial_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                            const float* x, const int64_t* y, int32_t loss_kind, float* z,
                            float* loss_terms, int64_t B, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Calibrator.predict of a radial flow calibrator, per row:
 *   xc = x - mean(x);  z = radial stack(xc);  p = softmax(z)
 *   probs = softmax(log(p + 1e-7) - log_priors)
 * in one pass that keeps the row in registers.  log_priors [D] DEVICE floats;
 * probs [B][D].  Envelope, workspace, prepare launch, validation, B == 0 rule
 * and determinism as cnf_radial_forward. */
int cnf_radial_predict(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, const float* log_priors, float* probs, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The score variant of cnf_radial_predict, as cnf_planar_score is of
 * cnf_planar_predict: ONE launch that ADDS into `record` the words that
 * cnf_radial_predict followed by cnf_metrics(probs, y, ...) would leave; the
 * probabilities are never stored.  Validation is the sibling's plus
 * cnf_metrics' (2 <= dim, bins in 1..CNF_MAX_BINS, B <= 2^26, y and record
 * 8-byte aligned, record non-NULL), all before any HIP call.  B == 0 returns
 * CNF_OK without a launch and leaves the record as it is. */
int cnf_radial_score(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                     const float* log_priors, const int64_t* y, int32_t bins, int64_t* record,
                     int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Reverse mode of cnf_radial_forward: upstream gz [B][D], gz_all [L][B][D]
 * (each may be NULL = zero); writes grads [cnf_radial_param_count] (per layer
 * z0, a, b; overwritten) and dx [B][D] (may be NULL).  The forward pass is
 * recomputed inside; the only tape is one r per (row, layer), from which a
 * layer's input is rebuilt as z0 + (z - z0) (a + r) / (r + sp); above 10
 * layers the row is also run forward again from x every 16 layers, so no input
 * comes out of more than 16 such inversions.  The norm's gradient is 0 where
 * r == 0, as torch's. */
int cnf_radial_vjp(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                   const float* gz, const float* gz_all, float* grads, float* dx, int64_t B,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Fused forward + loss + reverse mode, as cnf_planar_loss_vjp without `det`:
 * loss_terms[3] (sums over this batch, the third 0), grads = grad_scale *
 * d(sum of the per-row loss)/d(params), dx [B][D] likewise, may be NULL. */
int cnf_radial_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                        const float* x, const int64_t* y, int32_t loss_kind, float grad_scale,
                        float* loss_terms, float* grads, float* dx, int64_t B, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Affine-constant flows: a Flow of the reference's AffineConstantLayers
 * (flows/flows.py:40-65; train-flows-det.ipynb, AffineConstantFlow), each with
 * both parameters s [1][D], t [1][D] (that state_dict order):
 *   forward  z = x * exp(s) + t,    log_det = sum_d s     (one number, not per row)
 *   inverse  x = (z - t) * exp(-s), log_det = sum_d -s
 * A layer rounds as torch's ops do (product, then sum; difference, then
 * product) and the layers are applied one after another, never composed.  The
 * stack's log-det is an fp32 sum over d per layer, then 0 + ld_0 + ld_1 + ...
 * in the direction's layer order, formed once per call: logdet / gld below are
 * [1] DEVICE floats and may be NULL.  All fp32.
 *   dim       D, 1..CNF_MAX_DIM;  n_layers  L, 1..CNF_AFFINE_MAX_LAYERS
 *             (< 1: CNF_ERR_DESC; above: CNF_ERR_UNSUPPORTED)
 *   params    HOST array of 2 * L DEVICE pointers: s, t of layer 0, 1, ...
 *             (non-NULL, 4-byte aligned)
 *   B         0..2^31 rows (CNF_ERR_BATCH otherwise)
 *   workspace cnf_affine_workspace_bytes(dim, n_layers, B) bytes of DEVICE
 *             memory, no initialisation needed; one size serves every entry
 *             point.  A call first writes each layer's (exp(+-s), t, log-det)
 *             there with one small launch, so nothing is cached between calls.
 * In floats, with LPR, DP, r64, F and U as for the planar family and
 * PW = L * 2 D + 4, the workspace holds
 *   r64(L * (2 DP + 8)) + r64(PW) + r64(max(U * PW, 4 * F))
 * There is no per-row tape: the reverse mode keeps each layer's input in
 * registers up to 10 layers, and above keeps every 16th and runs the row
 * forward from it (a layer's input is never rebuilt by inverting the layer).
 * Argument errors, the B == 0 rule (memset nodes only), determinism and the
 * absence of atomics, allocation and host synchronisation are the planar
 * family's.  A deliberate limit of B == 0: the log-det does not depend on the
 * rows, but no kernel runs to form it, so logdet is ZEROED (not sum_d s) and
 * cnf_affine_vjp zeroes grads without adding gld to the s entries; a caller
 * that needs either for an empty batch forms it itself (cnf_hip/affine.py
 * does, with torch ops). */
#define CNF_AFFINE_MAX_LAYERS 64

/* 2 * L tensors, 2 * L * D floats. */
int cnf_affine_param_count(int32_t dim, int32_t n_layers, int64_t* n_floats);
int cnf_affine_workspace_bytes(int32_t dim, int32_t n_layers, int64_t B, size_t* bytes);
/* As cnf_planar_launch_plan; regt: every layer's input in registers (L <= 10);
 * rega: LPR == 1 and D <= 10 at L <= 10. */
int cnf_affine_launch_plan(int32_t dim, int32_t n_layers, int64_t B, int32_t out[8]);

/* Flow.forward of the stack: z [B][D] (= zs[-1]), logdet [1], z_all [L][B][D]
 * (the zs list); each may be NULL. */
int cnf_affine_forward(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, float* z, float* logdet, float* z_all, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Flow.backward of the stack (the INVERSE transform): x [B][D] (= xs[-1]),
 * logdet [1] (the sum of -sum_d s from the last layer to the first), x_all
 * [L][B][D] with x_all[k] the rows after undoing layer L-1-k (the xs list);
 * each may be NULL.  There is no reverse mode of the inverse. */
int cnf_affine_inverse(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* z, float* x, float* logdet, float* x_all, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Forward + loss terms, as cnf_planar_forward_loss: the per-row loss is
 * -(log(softmax(z)[y] + 1e-7) + ld) for CNF_LOSS_CAL and ce - det * ld for
 * CNF_LOSS_CE; loss_terms[3] = {sum of per-row loss, sum of ce, B * ld}; z and
 * logdet [1] may be NULL.  A label outside [0, D) makes the terms NaN. */
int cnf_affine_forward_loss(int32_t dim, int32_t n_layers, const float* const* params,
                            const float* x, const int64_t* y, int32_t loss_kind, float det,
                            float* z, float* logdet, float* loss_terms, int64_t B,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Calibrator.predict of an affine flow calibrator, per row:
 *   xc = x - mean(x);  z = affine stack(xc);  p = softmax(z)
 *   probs = softmax(log(p + 1e-7) - log_priors)
 * in one pass that keeps the row in registers.  log_priors [D] DEVICE floats;
 * probs [B][D].  Envelope, workspace, prepare launch, validation, B == 0 rule
 * and determinism as cnf_affine_forward. */
int cnf_affine_predict(int32_t dim, int32_t n_layers, const float* const* params,
                       const float* x, const float* log_priors, float* probs, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The score variant of cnf_affine_predict, as cnf_planar_score is of
 * cnf_planar_predict: ONE launch that ADDS into `record` the words that
 * cnf_affine_predict followed by cnf_metrics(probs, y, ...) would leave; the
 * probabilities are never stored.  Validation is the sibling's plus
 * cnf_metrics' (2 <= dim, bins in 1..CNF_MAX_BINS, B <= 2^26, y and record
 * 8-byte aligned, record non-NULL), all before any HIP call.  B == 0 returns
 * CNF_OK without a launch and leaves the record as it is. */
int cnf_affine_score(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                     const float* log_priors, const int64_t* y, int32_t bins, int64_t* record,
                     int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Reverse mode of cnf_affine_forward: upstream gz [B][D], gz_all [L][B][D],
 * gld [1] (each may be NULL = zero); writes grads [cnf_affine_param_count]
 * (per layer s, t; overwritten) and dx [B][D] (may be NULL).  With G_l the
 * gradient at layer l's output: grad t_l = sum_rows G_l, grad s_l = sum_rows
 * G_l z_{l-1} exp(s_l) + gld, G_{l-1} = G_l exp(s_l). */
int cnf_affine_vjp(int32_t dim, int32_t n_layers, const float* const* params, const float* x,
                   const float* gz, const float* gz_all, const float* gld, float* grads,
                   float* dx, int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* Fused forward + loss + reverse mode, as cnf_planar_loss_vjp: loss_terms[3]
 * (sums over this batch), grads = grad_scale * d(sum of the per-row loss)/
 * d(params), dx [B][D] likewise, may be NULL. */
int cnf_affine_loss_vjp(int32_t dim, int32_t n_layers, const float* const* params,
                        const float* x, const int64_t* y, int32_t loss_kind, float det,
                        float grad_scale, float* loss_terms, float* grads, float* dx, int64_t B,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Mixed row-wise flows: a Flow whose layers are PlanarLayers, RadialLayers and
 * AffineConstantLayers (both parameters) of one width D, in any order, as ONE
 * fused stack.  kinds: a HOST array of n_layers words, CNF_LAYER_PLANAR /
 * CNF_LAYER_RADIAL / CNF_LAYER_AFFINE per layer.  Each layer is computed
 * exactly as its own family documents it above (planar u_hat / tanh / log-det,
 * radial h = 1 / (a + r), affine a rounded product followed by a rounded sum);
 * the stack is never algebraically collapsed.  All fp32.
 *   dim       D, 1..CNF_MAX_DIM;  n_layers  L, 1..CNF_MIXED_MAX_LAYERS
 *             (< 1: CNF_ERR_DESC; above: CNF_ERR_UNSUPPORTED)
 *   kinds     NULL: CNF_ERR_NULL; a value outside 0..2: CNF_ERR_DESC.  A stack
 *             of a single kind is valid.
 *   params    HOST array of DEVICE pointers in layer order, each layer's
 *             tensors in its family's order: planar w, u, b; radial z0, a, b;
 *             affine s, t -- 3 or 2 entries per layer (non-NULL, 4-byte aligned)
 *   grads     flat in the same order (the state_dict order): 2 D + 1, D + 2 or
 *             2 D floats per layer
 *   logdet    [B], a row's: 0, then one rounded fp32 addition per planar layer
 *             (that row's term) and per affine layer (its sum_d s, an fp32 sum
 *             over d), in layer order, as Flow.forward accumulates it; a
 *             radial layer adds nothing
 *   gld       [B], a row's; an affine layer's grad s takes sum_rows gld
 *   B         0..2^31 rows (CNF_ERR_BATCH otherwise)
 *   workspace cnf_mixed_workspace_bytes(dim, n_layers, kinds, B) bytes of
 *             DEVICE memory, no initialisation needed; one size serves every
 *             entry point.  A call first writes one constant record of
 *             2 DP + 8 floats per layer there with one small launch.
 * In floats, with LPR, DP, r64, F and U as for the planar family and
 * PW = L * (2 D + 2) + 4, the workspace holds
 *   r64(L * (2 DP + 8)) + r64(PW) + r64(max(U * PW, 4 * F))
 * There is no per-row tape and no layer is ever inverted (a contracting affine
 * layer loses its input; a chain of radial inversions grows the error): the
 * reverse mode keeps each layer's input in registers up to 10 layers, and
 * above keeps every 16th and runs the row forward from it.
 * Order of the checks, all before any HIP call: shape; kinds (NULL, then each
 * value); for cnf_mixed_score the scoring arguments (as cnf_planar_score);
 * batch; the parameter table entry by entry (NULL, then alignment); x /
 * workspace NULL or short; x / workspace alignment; then per kind of call --
 * forward: loss kind, loss NULLs, loss alignment, output alignment; reverse:
 * grads NULL, the loss checks, alignment; predict and score: NULLs, alignment.
 * B == 0 zeroes loss_terms / grads with memset nodes and launches no kernel.
 * Deterministic as the planar family: per-block partial sums added in block
 * order by a one-block follow-up launch, so two calls agree bitwise.  No float
 * atomics, no allocation, no host synchronisation. */
#define CNF_LAYER_PLANAR 0
#define CNF_LAYER_RADIAL 1
#define CNF_LAYER_AFFINE 2
#define CNF_MIXED_MAX_LAYERS 64

/* The sum over the layers of 2 D + 1 (planar), D + 2 (radial), 2 D (affine). */
int cnf_mixed_param_count(int32_t dim, int32_t n_layers, const int32_t* kinds, int64_t* n_floats);
int cnf_mixed_workspace_bytes(int32_t dim, int32_t n_layers, const int32_t* kinds, int64_t B,
                              size_t* bytes);
/* As cnf_planar_launch_plan; regt: every layer's input in registers (L <= 10,
 * and D <= 10 or D > 16); rega: regt and LPR == 1; gacc: PW > 3072.  Without
 * regt the reverse kernel is the checkpointed <LPR, CPL, 0, 0> instantiation. */
int cnf_mixed_launch_plan(int32_t dim, int32_t n_layers, const int32_t* kinds, int64_t B,
                          int32_t out[8]);

/* The entry points below are their cnf_planar_* siblings with `kinds` after
 * n_layers: the same arguments, outputs, NULL rules, loss kinds and `det`. */
int cnf_mixed_forward(int32_t dim, int32_t n_layers, const int32_t* kinds,
                      const float* const* params, const float* x, float* z, float* logdet,
                      float* z_all, int64_t B, void* workspace, size_t workspace_bytes,
                      void* stream);
/* loss_terms[3] = {sum loss, sum ce, sum ld} over the rows. */
int cnf_mixed_forward_loss(int32_t dim, int32_t n_layers, const int32_t* kinds,
                           const float* const* params, const float* x, const int64_t* y,
                           int32_t loss_kind, float det, float* z, float* logdet,
                           float* loss_terms, int64_t B, void* workspace, size_t workspace_bytes,
                           void* stream);
/* As cnf_planar_predict word for word: centring, both softmaxes, the prior
 * correction; logdet [B] of the centred rows, may be NULL. */
int cnf_mixed_predict(int32_t dim, int32_t n_layers, const int32_t* kinds,
                      const float* const* params, const float* x, const float* log_priors,
                      float* probs, float* logdet, int64_t B, void* workspace,
                      size_t workspace_bytes, void* stream);
/* As cnf_planar_score: ONE launch that ADDS into `record` the words that
 * cnf_mixed_predict followed by cnf_metrics(probs, y, ...) would leave. */
int cnf_mixed_score(int32_t dim, int32_t n_layers, const int32_t* kinds,
                    const float* const* params, const float* x, const float* log_priors,
                    const int64_t* y, int32_t bins, int64_t* record, int64_t B, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Reverse mode of cnf_mixed_forward: upstream gz [B][D], gz_all [L][B][D], gld
 * [B] (each may be NULL = zero); writes grads [cnf_mixed_param_count]
 * (overwritten) and dx [B][D] (may be NULL). */
int cnf_mixed_vjp(int32_t dim, int32_t n_layers, const int32_t* kinds,
                  const float* const* params, const float* x, const float* gz,
                  const float* gz_all, const float* gld, float* grads, float* dx, int64_t B,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Fused forward + loss + reverse mode, as cnf_planar_loss_vjp. */
int cnf_mixed_loss_vjp(int32_t dim, int32_t n_layers, const int32_t* kinds,
                       const float* const* params, const float* x, const int64_t* y,
                       int32_t loss_kind, float det, float grad_scale, float* loss_terms,
                       float* grads, float* dx, int64_t B, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Which kernel family serves this descriptor's launches: "sgpr-fused"
 * (pipelined scalar weights, every output mode), "valu-fused" (strict_nan,
 * shapes whose Linears exceed 32 floats, misaligned views), "mfma-wide"
 * (register-resident MFMA, the wide shapes of its table), "mfma-tile" (other
 * wide shapes, every-layer outputs of wide stacks). */
const char* cnf_kernel_name(const cnf_desc* desc);

/* Which reverse-mode path serves cnf_vjp / cnf_loss_vjp for this descriptor
 * (host only, no launch): "vjp2" (packed-pair scalar-weight kernel, one launch),
 * "vjp-rows" (row-resident kernel, one launch), "layerwise" (layer-at-a-time
 * MFMA sweeps), "wide-fused" (the fused training sweeps of the mfma-wide
 * shapes; judged at B = 1, a tape beyond the sweeps' limit runs layerwise) or
 * "none" (cnf_vjp_workspace_bytes returns CNF_ERR_UNSUPPORTED, and for an
 * invalid descriptor). */
const char* cnf_vjp_kernel_name(const cnf_desc* desc);

/* What cnf_vjp / cnf_loss_vjp (inverse = 0) or cnf_vjp_inverse (inverse = 1)
 * launches for this descriptor on B rows (host only, no HIP call), every word
 * computed by the function the launch itself uses.  B == 0 reports B == 1 (no
 * kernel runs).  out[0] is the path, judged at B (cnf_vjp_kernel_name judges
 * wide-fused at B = 1); words a path does not name are 0.
 *   layerwise (the inverse's reverse mode is always layerwise):
 *     [1] kNJ of k_wfwd_update / k_wbwd_update (0 for the inverse, whose update
 *         kernels loop over the columns), [2] keep_acts (0: the backward sweep
 *         recomputes the conditioner activations), [3] nkb row blocks of the
 *         weight gradients, [4] rows per block, [5] k_wseed blocks, [6] blocks
 *         of the one-wave-per-row kernels, [7] k_wdw16's grid z,
 *     [8] the k_wgemm instantiations of a layer's sweeps, bit 2 f + (NC - 1)
 *         with f the (BT, EPI, PAIR) form: 0 forward bias, 1 forward bias +
 *         activation, 2 back-prop with the activation's derivative, 3 the
 *         first Linear's back-prop of both nets (PAIR), 4 of one net,
 *     [9] the most column blocks (ny) and [10] the most reduction chunks of
 *         128 over those launches.  Words 7-10 are 0 without a conditioner.
 *   wide-fused:
 *     [1] the row of k_wide16's table, [2] nets, [3] nkb, [4] rows per block,
 *     [5] k_wseed blocks (generic seeds), [6] 1: the weight gradients run on
 *     k_wdw16g, 0: on k_wdw16 with [7] its grid z, [8] the k_wdw16g classes
 *     (G tiles, H tiles) of the layer's jobs, bit i the i-th class of
 *     (7,4) (7,7) (4,7) (4,4) (4,2) (4,5) (1,5).
 * Errors as cnf_vjp_workspace_bytes, except that an unsupported reverse mode
 * is CNF_OK with path CNF_VJP_PATH_NONE; inverse outside {0, 1}: CNF_ERR_DESC. */
#define CNF_VJP_PLAN_WORDS 16
enum {
  CNF_VJP_PATH_NONE = 0,
  CNF_VJP_PATH_VJP2 = 1,
  CNF_VJP_PATH_ROWS = 2,
  CNF_VJP_PATH_LAYERWISE = 3,
  CNF_VJP_PATH_WIDE_FUSED = 4
};
int cnf_vjp_launch_plan(const cnf_desc* desc, int64_t B, int32_t inverse,
                        int32_t out[CNF_VJP_PLAN_WORDS]);

const char* cnf_strerror(int status);
/* The hipError_t behind the last CNF_ERR_HIP on this thread. */
int cnf_last_hip_error(void);
int cnf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CNF_H_ */
