/*
 * bgp.h -- C-ABI of the MI355X-native BayesGPR hot path (libbgp.so).
 *
 * The reference (kiudee/bayes-skopt 0.11.0) has no FFI boundary: the seams this library sits
 * behind are Python call sites.  Each entry point below names the
 * reference interface it replaces.  The host side that binds these symbols with ctypes lives in
 * bayes-skopt_amd/_lib.py; INTEGRATION.md shows the stub a bask maintainer would add.
 *
 * Conventions
 *  - plain C types only; all host buffers are caller-owned, C-contiguous, fp64 (double) / int32;
 *  - return value 0 == BGP_OK, anything else is an error whose text bgp_last_error() returns
 *    (thread-local); no C++ exception crosses the ABI;
 *  - NUMERICAL failures (non-positive pivot == "not positive definite") are per-item:
 *    status[b] != 0 and lml[b] = -inf  (sklearn/_gpr.py:586-589 returns -inf there), never a
 *    call failure;
 *  - hyper-parameters are passed in the CANONICAL log-space layout
 *        h = [ log c, log l_1 .. log l_d, log s2 ]            (d + 2 doubles per item)
 *    with   K = c * S(r) + s2 * I   (form BGP_FORM_PRODUCT; ConstantKernel * Matern + WhiteKernel,
 *                                    bask/utils.py:144-150 + skopt's added WhiteKernel)
 *           K = c + S(r) + s2 * I   (form BGP_FORM_SUM;     examples/Fit-GP.ipynb cell 6)
 *    r_ij^2 = sum_k ((x_ik - x_jk) / l_k)^2 ; -inf encodes an absent / zeroed component
 *    (bask/bayesgpr.py:328-333 swaps in WhiteKernel(0.0)).  The mapping from a kernel object's
 *    theta (sklearn/kernels.py:733-760 concatenation order, fixed hyper-parameters dropped,
 *    isotropic length scale replicated) to h is host logic (bayes-skopt_amd/kernels.py);
 *  - one context per (host thread, device); calls on a context are serialised on its HIP stream.
 */
#ifndef BGP_H
#define BGP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGP_OK 0
#define BGP_ERR_INVALID 1  /* bad argument                      */
#define BGP_ERR_HIP 2      /* a HIP runtime call failed          */
#define BGP_ERR_NODEVICE 3 /* no usable gfx950 device            */
#define BGP_ERR_STATE 4    /* call order (e.g. predict before posterior) */
#define BGP_ERR_NOTPD 5    /* bgp_sample_y: covariance (+jitter) not positive definite */
#define BGP_ERR_COMM 6     /* a collective did not complete (peer lost, asynchronous RCCL error): communicator aborted */

enum { BGP_FORM_PRODUCT = 0, BGP_FORM_SUM = 1 };
enum { BGP_RBF = 0, BGP_MATERN12 = 1, BGP_MATERN32 = 2, BGP_MATERN52 = 3 };

typedef struct bgp_kernel_spec {
  int form;       /* BGP_FORM_*                                   */
  int stationary; /* BGP_RBF / BGP_MATERN*  (sklearn/kernels.py:1553-1560, 1713-1733) */
  int d;          /* input dimension                              */
} bgp_kernel_spec;

typedef struct bgp_ctx bgp_ctx;

/* Number of visible HIP devices (0 when none / runtime unusable). */
int bgp_device_count(void);
/* PCI bus id ("0000:05:00.0") of visible device `device` into buf (len >= 16): the identity that tells apart ranks which a
 * launcher has pinned to one GPU each through HIP_VISIBLE_DEVICES -- they all see "device 0" (bayes-skopt_amd/distributed.py). */
int bgp_device_pci_bus_id(int device, char* buf, int len);
/* Text of the last error on this thread. */
const char* bgp_last_error(void);
/* Library version string. */
const char* bgp_version(void);

/*
 * Create a context on `device` holding the training set (copied to HBM and kept resident):
 * X (n*d row-major), y (n, already normalised by the caller as bask/bayesgpr.py:470-478 does),
 * alpha_diag (n; the diagonal term sklearn/_gpr.py:585 adds -- scalar alpha already broadcast,
 * noise vector already added, bask/bayesgpr.py:338-349).
 * max_batch bounds the number of hyper-parameter vectors factorised concurrently (workspace is
 * max_batch * n_pad^2 doubles); larger B are processed in chunks.
 * Replaces: the data the reference keeps on self.X_train_/y_train_/alpha (bask/bayesgpr.py:485-488).
 */
int bgp_ctx_create(int device, int n, int d, const double* X, const double* y, const double* alpha_diag,
                   const bgp_kernel_spec* ks, int max_batch, bgp_ctx** out);

/* tell() grows the data set (bask/optimizer.py:288-320 -> bask/bayesgpr.py:469-488). d is fixed. */
int bgp_ctx_update_data(bgp_ctx* ctx, int n, const double* X, const double* y, const double* alpha_diag);

void bgp_ctx_destroy(bgp_ctx* ctx);

/*
 * Batched log-marginal-likelihood: for each of B canonical vectors h_b
 *     K_b = kernel(X) ; K_b[diag] += alpha_diag ; L_b = chol(K_b) ;
 *     lml_b = -1/2 y^T K_b^-1 y - sum log diag(L_b) - n/2 log(2 pi)
 * Replaces: GaussianProcessRegressor.log_marginal_likelihood(theta) (sklearn/_gpr.py:537-613)
 * as called per walker by BayesGPR._log_prob_fn (bask/bayesgpr.py:374) from
 * emcee.EnsembleSampler.compute_log_prob (bask/bayesgpr.py:510-524).
 * status[b] = 0 ok, >0 = 1-based index of the failing pivot (lml[b] = -inf). status may be NULL.
 */
int bgp_lml_batch(bgp_ctx* ctx, int B, const double* h, double* lml, int* status);

/*
 * Input warping (bask/bayesgpr.py:249-316, warp_inputs=True): every input column k is passed through the
 * CDF of Beta(exp(wa_k), exp(wb_k)) before the kernel is evaluated.  warp vectors are 2*d doubles in log
 * space, [wa_1..wa_d, wb_1..wb_d] -- the tail the reference appends to theta (bask/bayesgpr.py:355-357).
 *
 * bgp_lml_batch_warped: as bgp_lml_batch, but walker b sees the design matrix through its own warp
 *   warp[b*2d .. (b+1)*2d).  Replaces create_warpers() + rewarp() + log_marginal_likelihood per walker
 *   (bask/bayesgpr.py:353-374).
 * bgp_ctx_set_warp: context-level warp (the geometric-median warpers, bask/bayesgpr.py:535-541) seen by
 *   every later posterior / predict / pvrs / gradient / sample_y / bgp_lml_batch call, including their
 *   query points (bask/bayesgpr.py:630-632); NULL clears it; bgp_ctx_update_data clears it.
 * bgp_beta_cdf: warp m points (m*d row-major) on the device -- BayesGPR.warp() (bask/bayesgpr.py:249-264).
 *
 * Domain and accuracy of the Beta CDF (all three entry points and the resident sampler's warped walkers run one kernel):
 *   log-space parameters |w| <= 15, i.e. a, b in [3.1e-7, 3.3e6].  There the continued fraction converges within its 1000
 *   iterations at every x.  The error is ABSOLUTE (a warped coordinate lives in [0, 1] and enters the kernel through
 *   differences): 8 eps (1 + |lgamma(a+b)| + |lgamma(a)| + |lgamma(b)| + |a log x| + |b log1p(-x)|), which is 2e-15 for
 *   |w| <= 1, 3e-14 for |w| <= 4 and 2e-13 for |w| <= 6 (tests/_warpref.py); the relative error of a small result above the
 *   switch point (a+1)/(a+b+2) reaches 1e-10 at |w| = 6.  x <= 0 gives exactly 0, x >= 1 exactly 1.
 *   Outside the domain nothing wrong is handed on as a number: a parameter whose exp is 0, inf or NaN gives NaN at every x,
 *   and so does a continued fraction that has not converged (first between |w| = 15.7 and 15.8).  bgp_beta_cdf returns those
 *   NaNs; a Gram matrix built from them fails its factorisation, so bgp_lml_batch_warped answers lml = -inf with a non-zero
 *   status for that row (the other rows keep their bits) and the resident sampler rejects the proposal.
 *
 * Per-row-warped posteriors (bgp_posterior_batch_warped, below): posterior b is built from the un-warped training inputs
 *   through ITS OWN warp and keeps them resident; a context-level warp is replaced for that call, not composed.  While such
 *   posteriors are resident only bgp_predict_batch_warped and bgp_predict_mixture_warped read them (and bgp_cross_validate, which needs neither the inputs nor
 *   the kernel): every entry point that would combine resident posteriors
 *   with the context's shared (warped or un-warped) training inputs -- bgp_predict_batch, bgp_acq_batch, bgp_sample_y,
 *   bgp_sample_y_batch, bgp_pvrs, bgp_fantasy_begin, bgp_predict_grad_batch, bgp_minimize_starts, bgp_paths_begin,
 *   bgp_partial_dependence, bgp_sobol_indices, bgp_grad_cov, bgp_knowledge_gradient, bgp_joint_entropy, bgp_predict_mixture -- returns BGP_ERR_STATE and launches nothing.  Any posterior build (bgp_posterior_batch*,
 *   bgp_pvrs_prepare, bgp_lml_grad_batch), bgp_ctx_set_warp and bgp_ctx_update_data end that state.
 */
int bgp_lml_batch_warped(bgp_ctx* ctx, int B, const double* h, const double* warp, double* lml, int* status);
int bgp_ctx_set_warp(bgp_ctx* ctx, const double* warp);
int bgp_beta_cdf(bgp_ctx* ctx, int m, const double* X, const double* warp, double* out);

/*
 * Asynchronous bgp_lml_batch (B <= max_batch): submit enqueues the whole batch on the device and returns, wait blocks
 * until it is done and hands back lml / status (status may be NULL); with per-launch timing on (bgp_set_timing) submit
 * returns BGP_ERR_STATE (the timed path synchronises inside bgp_lml_batch).  Between the two calls the host is free -- the
 * sampler evaluates the log-priors of the same proposals there (bask/bayesgpr.py:366-372 runs them back to back).
 * One batch may be pending per context, and it owns the workspace: until wait has collected it every other entry point
 * that computes on the context returns BGP_ERR_STATE.  Proposals and results travel through pinned host memory; same
 * results as bgp_lml_batch (which takes this path itself for a single chunk).
 */
int bgp_lml_batch_submit(bgp_ctx* ctx, int B, const double* h);
/* the same for per-walker warps (the asynchronous form of bgp_lml_batch_warped; bask/bayesgpr.py:353-374) */
int bgp_lml_batch_warped_submit(bgp_ctx* ctx, int B, const double* h, const double* warp);
int bgp_lml_batch_wait(bgp_ctx* ctx, double* lml, int* status);

/*
 * LML and its gradient w.r.t. the canonical vector (grad is B*(d+2)):
 *     g_k = 1/2 tr((alpha alpha^T - K^-1) dK/dh_k)
 * Replaces: log_marginal_likelihood(theta, eval_gradient=True) (sklearn/_gpr.py:615-647,
 * kernels.py:1746-1766) driven by L-BFGS-B inside fit (bask/bayesgpr.py:607).
 */
int bgp_lml_grad_batch(bgp_ctx* ctx, int B, const double* h, double* lml, double* grad, int* status);

/*
 * Parity helper: the jittered Gram matrix K(h) itself, n*n row-major (both triangles filled).
 * Replaces: kernel_(X_train_) + diagonal add (bask/bayesgpr.py:203-204).
 */
int bgp_kernel_matrix(bgp_ctx* ctx, const double* h, double* K);

/*
 * Posterior build for B hyper-posterior samples; factors stay RESIDENT on the device for the
 * predict / pvrs calls that follow.  Any of the output pointers may be NULL.
 *   L      B*n*n row-major lower Cholesky factors (upper triangle zero)   -> BayesGPR.L_
 *   alpha  B*n            K^-1 y                                          -> BayesGPR.alpha_
 *   K_inv  B*n*n          explicit inverse                                -> BayesGPR.K_inv_
 * Replaces: the BayesGPR.theta setter (bask/bayesgpr.py:200-217), called once per sample()
 * (:544) and once per hyper-posterior sample by evaluate_acquisitions (bask/acquisition.py:112-121).
 */
int bgp_posterior_batch(bgp_ctx* ctx, int B, const double* h, double* L, double* alpha, double* K_inv,
                        double* lml, int* status);

/*
 * Predict at m query points with the B resident posteriors.  h_kernel (B*(d+2)) are the
 * hyper-parameters currently in kernel_ -- they differ from the posterior's only inside
 * noise_set_to_zero() (log s2 = -inf), which does NOT rebuild the factors
 * (bask/bayesgpr.py:318-336).  Outputs (normalised-y units; the caller undoes y
 * normalisation): mean B*m, var B*m (clipped at 0), optional cov B*m*m (may be NULL).
 *   mean = K_* alpha ; var = k_** - diag(K_* K^-1 K_*^T) ; cov = K_** - K_* K^-1 K_*^T
 * Replaces: BayesGPR.predict (bask/bayesgpr.py:622-635 -> skopt predict).
 */
int bgp_predict_batch(bgp_ctx* ctx, int B, const double* h_kernel, int m, const double* Xq, double* mean,
                      double* var, double* cov);

/*
 * The same pair for hyper-posterior draws under input warping, where every draw carries its own warp and therefore its own
 * training inputs (evaluate_acquisitions under warp_inputs: create_warpers + rewarp + theta setter + predict per chain row,
 * bask/acquisition.py:112-125,142-145).
 *   bgp_posterior_batch_warped  as bgp_posterior_batch, item b built from the training inputs through warp[b*2d .. (b+1)*2d)
 *          (log space, [wa_1..wa_d, wb_1..wb_d] as for bgp_lml_batch_warped).  The B warped design matrices and the warp
 *          parameters stay resident beside K^-1 / alpha; a warped LML batch in between does not touch them.  Same chunking,
 *          outputs and status semantics: a matrix that is not positive definite fails alone.
 *   bgp_predict_batch_warped    as bgp_predict_batch without cov: item b sees the m query rows through its own warp (one upload,
 *          one warp launch over the B parameter sets) and its own warped training inputs.  Needs B <= the resident posteriors of
 *          a bgp_posterior_batch_warped call, BGP_ERR_STATE otherwise.
 * Item b's results are the bits of bgp_ctx_set_warp(warp_b) + bgp_posterior_batch(h_b) + bgp_predict_batch(h_kernel_b).
 */
int bgp_posterior_batch_warped(bgp_ctx* ctx, int B, const double* h, const double* warp, double* L, double* alpha,
                               double* K_inv, double* lml, int* status);
int bgp_predict_batch_warped(bgp_ctx* ctx, int B, const double* h_kernel, int m, const double* Xq, double* mean, double* var);

/*
 * Closed-form acquisition functions averaged over the B resident posteriors (hyper-posterior draws), evaluated
 * on the device right behind the batched predict so that the B*m means and variances never cross PCIe.
 * For acquisition k (kinds[k], params[k]) and draw b, with mu = y_std * mean + y_mean, std = sqrt(var * y_std^2):
 *   BGP_ACQ_EI    std * (x Phi(x) + phi(x)), x = (y_opt - mu) / std, 0 where std <= 0; y_opt = params[k], or the
 *                 draw's lowest mu when params[k] is NaN          (bask/acquisition.py:154-172)
 *   BGP_ACQ_MEAN  -mu                                              (Expectation, :197-201)
 *   BGP_ACQ_LCB   params[k] * std - mu                             (LCB, :204-216)
 *   BGP_ACQ_STD   std                                              (LCB with alpha = "inf")
 * out[k*m + i] = sum over the draws, in order, of value / n_samples; a draw whose values are not all finite
 * contributes nothing (evaluate_acquisitions, bask/acquisition.py:112-139).  h_kernel as in bgp_predict_batch.
 * bgp_acq_values applies the same closed forms to caller-supplied mu / std (B*m each, y units).
 */
enum { BGP_ACQ_EI = 0, BGP_ACQ_MEAN = 1, BGP_ACQ_LCB = 2, BGP_ACQ_STD = 3 };
#define BGP_ACQ_MAX 8
int bgp_acq_batch(bgp_ctx* ctx, int B, const double* h_kernel, int m, const double* Xq, double y_mean, double y_std,
                  int n_acq, const int* kinds, const double* params, int n_samples, double* out);
int bgp_acq_values(bgp_ctx* ctx, int B, int m, const double* mu, const double* std_, int n_acq, const int* kinds,
                   const double* params, int n_samples, double* out);

/*
 * The hyper-posterior mixture: the posterior predictive at a point with the kernel hyper-parameters integrated out,
 *   sum_b w^_b N(mu_b(x), sd_b(x)^2)  over B posteriors (chain rows),
 * evaluated on the device behind the batched predict (the B*m means and variances never cross PCIe).
 *   bgp_predict_mixture         the first B resident posteriors, as bgp_acq_batch; h_kernel as in bgp_predict_batch (the white
 *                               level is h_kernel's last entry: -inf for the latent function).  Its moments are made of the bits
 *                               bgp_predict_batch returns.
 *   bgp_predict_mixture_warped  the same on per-row-warped resident posteriors (bgp_posterior_batch_warped).
 *   bgp_mixture_values          the same pass on caller-supplied normalised mean / var (B*m each): generic kernel trees, more rows
 *                               than max_batch.  Needs no resident posterior.
 * With mu_bi = y_std * mean_bi + y_mean and sd_bi = sqrt(var_bi * (y_std * y_std)):
 *   weights (B, or NULL: w_b = 1).  Row b is USED iff w_b > 0 and all of its m means and variances are finite; W = sum of w_b over
 *   the used rows in ascending b, w^_b = w_b / W, *n_used = their count.  n_used == 0: every output is NaN, the call returns BGP_OK.
 *   moments (3*m, may be NULL): mean_i = sum w^_b mu_bi;  within_i = sum w^_b sd_bi^2;  between_i = sum w^_b (mu_bi - mean_i)^2 in a
 *     second pass against the finished mean (>= 0, exactly 0 for B = 1).  The predictive variance is within + between.
 *   at_t (3*m, may be NULL; needs t, one value per point, y units), z_bi = (t_i - mu_bi) / sd_bi:
 *     cdf_i = sum w^_b Phi(z_bi), sf_i = sum w^_b Phi(-z_bi), each tail summed on its own from erfc of a non-negative argument (a
 *     1e-300 tail keeps its relative accuracy);  logpdf_i = log sum w^_b exp(-z^2 / 2) / (sd_bi sqrt(2 pi)) as a max-shifted sum.
 *     A component with sd = 0 is a step at mu_bi (Phi = 1 where t >= mu, else 0) and adds nothing to the density; logpdf is -inf
 *     when no used component has sd > 0.
 *   quant (Q*m, may be NULL; Q <= BGP_MIX_QMAX probabilities probs inside (0, 1)): q_pi = inf {t : F_i(t) >= p}.  F = p is solved
 *     for p <= 0.5 and S = 1 - p above.  Bracket: [min_b, max_b] of mu_bi + z_p sd_bi over the used rows, z_p from the device's own
 *     inverse normal; an end whose evaluated sign is wrong moves outwards.  The bracket shrinks by safeguarded Newton steps (slope:
 *     the mixture density; bisection when a step leaves the bracket or the bracket has not halved in two steps) until its ends are
 *     adjacent doubles, and the UPPER end is returned: the result is deterministic and a quantile carried by an atom (sd = 0) is
 *     exactly that mu.  Iteration cap 200: the upper end of the bracket reached by then is returned.
 * Every sum runs over the used rows in ascending b, one thread per point: when no row is dropped a point's results are the same
 * bits alone and in a crowd.  A negative or non-finite weight, Q > BGP_MIX_QMAX or a probs entry outside (0, 1): BGP_ERR_INVALID.
 * bgp_mixture_stats: out[0] = the largest solver iteration count of the context's last mixture call, out[1] = the largest number
 * of bracket moves.
 */
#define BGP_MIX_QMAX 16
int bgp_predict_mixture(bgp_ctx* ctx, int B, const double* h_kernel, const double* weights, int m, const double* Xq, double y_mean,
                        double y_std, int Q, const double* probs, const double* t, double* moments, double* quant, double* at_t,
                        int* n_used);
int bgp_predict_mixture_warped(bgp_ctx* ctx, int B, const double* h_kernel, const double* weights, int m, const double* Xq,
                               double y_mean, double y_std, int Q, const double* probs, const double* t, double* moments,
                               double* quant, double* at_t, int* n_used);
int bgp_mixture_values(bgp_ctx* ctx, int B, int m, const double* mean, const double* var, const double* weights, double y_mean,
                       double y_std, int Q, const double* probs, const double* t, double* moments, double* quant, double* at_t,
                       int* n_used);
int bgp_mixture_stats(bgp_ctx* ctx, long long* out);

/*
 * PVRS inner loop with the resident posterior built by bgp_pvrs_prepare (K without the candidate
 * row):  for every candidate i
 *   covs[i] = sum_t k_t,aug^T K_aug,i^-1 k_t,aug ,   K_aug,i = kernel([X_train; x_i])
 * computed with the bordered-Cholesky identity instead of m factorizations.
 * Replaces: PVRS.__call__ loop (bask/acquisition.py:328-338); with thompson == candidates it is
 * VarianceReduction (bask/acquisition.py:287-300).
 */
int bgp_pvrs(bgp_ctx* ctx, const double* h_kernel, int m, const double* Xcand, int T, const double* Xthompson,
             double* covs);
/* Build the resident posterior bgp_pvrs needs: K = kernel_(X_train) (+ alpha_diag only when
 * has_alpha_vec != 0 -- the reference adds alpha to the augmented diagonal only when it is
 * iterable, bask/acquisition.py:332-333).  status (1 int, may be NULL) as in bgp_lml_batch. */
int bgp_pvrs_prepare(bgp_ctx* ctx, const double* h_kernel, int has_alpha_vec, int* status);

/*
 * Batch proposals by fantasy conditioning: Optimizer.ask(n_points > 1) (skopt's "constant liar" / kriging-believer
 * batches; bask/optimizer.py:177 has the signature and refuses).  The B resident posteriors of the proposal
 * (bgp_posterior_batch with the draws' h, built first) are conditioned one chosen candidate p at a time on a fantasy
 * observation, with the hyper-parameters and the y normalisation fixed:
 *   w_b = K_b^-1 k_b(X, x_p) ;  c_b(i) = k_b(x_i, x_p) - k_b(X, x_i)^T w_b - sum_{l<j} u_{b,l}(i) u_{b,l}(p)
 *   s_b = c_b(p) + noise[b] ;  u_{b,j} = c_b / sqrt(s_b) ;  var_b -= u_{b,j}^2 ;  mu_b += u_{b,j} (lie_b - mu_b(p)) / sqrt(s_b)
 * -- the latent predictive moments of the GP whose training set is X plus the chosen points with their lies (each with
 * noise variance noise[b]: the constructor's scalar alpha + the draw's white level), i.e. what
 * evaluate_acquisitions (bask/acquisition.py:112-139) would see after tell(chosen, lies) without a refit.
 * bgp_fantasy_begin: h_kernel (B*(d+2)) as in bgp_acq_batch (white level -inf), noise (B), the m candidates, the
 *   acquisitions (kinds / params / n_samples as bgp_acq_batch) and qmax < m, the largest number of steps; the starting
 *   moments are bgp_predict_batch's.  Needs d <= 32 and no context-level warp.
 * bgp_fantasy_step: condition on candidate p with lie_kind BGP_LIE_VALUE (every draw's lie is lie_value, normalised-y
 *   units: cl_min / cl_mean / cl_max) or BGP_LIE_KB (each draw's own mean at p: means unchanged); then the closed forms
 *   and the average over the draws exactly as bgp_acq_batch, and *next = the argmax of acquisition 0 over the candidates
 *   not chosen so far (np.argmax order).  values (n_acq*m, may be NULL): the averaged values.  BGP_ERR_STATE when the
 *   resident posteriors have been rebuilt since begin.
 * bgp_fantasy_moments: the current latent means / variances (B*m each, normalised units).
 * bgp_fantasy_end: drop the state (bgp_ctx_destroy drops it too).
 * bgp_fantasy_stats: out[0] = begins, out[1] = steps run on this context.
 */
enum { BGP_LIE_VALUE = 0, BGP_LIE_KB = 1 };
int bgp_fantasy_begin(bgp_ctx* ctx, int B, const double* h_kernel, const double* noise, int m, const double* Xcand,
                      double y_mean, double y_std, int n_acq, const int* kinds, const double* params, int n_samples, int qmax);
int bgp_fantasy_step(bgp_ctx* ctx, int p, int lie_kind, double lie_value, int* next, double* values);
int bgp_fantasy_moments(bgp_ctx* ctx, double* mean, double* var);
int bgp_fantasy_end(bgp_ctx* ctx);
int bgp_fantasy_stats(bgp_ctx* ctx, long long* out);

/*
 * Prediction gradients for any number of query rows, and the optimum search that stays on the device.
 * With G_i = d k(x, X_i) / dx (closed forms of kernel_.gradient_x for the four stationary families and both forms; the constant and
 * white terms contribute zeros; Matern 1/2: zero at r = 0):
 *   dmean = sum_i alpha_i G_i ;  dvar = -2 sum_i v_i G_i ,  v = K^-1 k(X, x)
 * bgp_predict_grad_batch: the B resident posteriors at m query rows; h_kernel as in bgp_predict_batch (white level -inf:
 *   noise_set_to_zero).  Outputs in normalised-y units: mean B*m, var B*m (clipped at 0), dmean B*m*d, dvar B*m*d (may be NULL).
 *   Replaces: skopt's GaussianProcessRegressor.predict(return_mean_grad, return_std_grad) for ONE point, reached from
 *   bask/bayesgpr.py:633; the reference raises for more than one row.
 * bgp_minimize_starts: minimise f(x) = y_mean + y_std mean(x) + kappa y_std sqrt(var(x)) over the box [lo, hi] (d doubles each) from
 *   the S starts X0 (S*d) with resident posterior b (h_kernel: its d + 2 kernel parameters); kappa = 0: the surrogate mean.  ONE
 *   launch, one workgroup per start running a projected BFGS iteration with Armijo backtracking (at most max_iter iterations of at
 *   most 30 trial points); where y_std sqrt(var) <= 1e-8 the std term contributes no gradient.  Per start: X_out (inside the box
 *   exactly), mean_out / var_out (normalised units: the bits bgp_predict_grad_batch returns at X_out), iters, evals (evaluations of f,
 *   the closing one at X_out included) and status -- 0: the inf-norm of the projected gradient of f (y units) is <= gtol, 1: max_iter
 *   reached, 2: the line search found no decrease, or f / its gradient is not finite at an iterate (a NaN start: X_out is the start).
 *   A start's result does not depend on the other starts.
 *   Replaces: the scipy L-BFGS-B loop of skopt.utils.expected_minimum (bask/optimizer.py:497-503).
 * Both need d <= 32 and no context-level warp (BGP_ERR_INVALID otherwise), and resident posteriors (BGP_ERR_STATE).
 */
int bgp_predict_grad_batch(bgp_ctx* ctx, int B, const double* h_kernel, int m, const double* Xq, double* mean, double* var,
                           double* dmean, double* dvar);
int bgp_minimize_starts(bgp_ctx* ctx, int b, const double* h_kernel, double y_mean, double y_std, double kappa, int S,
                        const double* X0, const double* lo, const double* hi, double gtol, int max_iter, double* X_out,
                        double* mean_out, double* var_out, int* iters, int* evals, int* status);

/*
 * Pathwise posterior function draws (Matheron's rule on random Fourier features): what BayesGPR.sample_y
 * (bask/bayesgpr.py:637-718) draws as a joint normal over the query set -- an m x m covariance and its factor per draw --, as
 * FUNCTIONS that cost O(F + n) per query row and can be evaluated anywhere, any number of times, consistently.  Serves the
 * Thompson draws of evaluate_acquisitions (bask/acquisition.py:132-136) and PVRS's Thompson points (bask/acquisition.py:328).
 * Path p (normalised-y units): resident posterior pidx[p]; kernel parameters h_kernel[p] (d + 2, white level -inf as in
 * bgp_predict_batch: a path is the latent function); s2[p] = the LOG white level of that posterior (-inf: none); host-drawn
 * omega[p] (F x d, from the spectral density of the unit-length-scale stationary part: N(0, I) for RBF, N(0, I) rows times
 * sqrt(2 nu / chi2_{2 nu}) for Matern nu), phase[p] (F, U[0, 2 pi)), w[p] (F + 1 standard normals, the last one the constant
 * term of the sum form) and eps[p] (n standard normals).  With A = sqrt(2 cS / F), cS = c (product form) or 1 (sum form):
 *   f0(x) = A sum_{j<F, ascending} w_j cos(phase_j + sum_k (x_k / l_k) omega_jk)  [+ sqrt(c) w_F, sum form]
 *   r = y - f0(X) - sqrt(alpha_diag + s2) eps ;  v = K^-1 r ;  f(x) = f0(x) + sum_{i, ascending} k(x, X_i) v_i
 *   df/dx_k = -A sum_j w_j sin(arg_j) omega_jk / l_k + sum_i v_i G_ik      (G as in bgp_predict_grad_batch)
 * bgp_paths_begin: build the state of P paths (1 .. 65 535) of F features (1 .. 65 536) -- omega / l, phase, A w, the constant
 *   term, v, copies of the training inputs and kernel parameters -- in one owned allocation; afterwards the paths do not read the
 *   resident posteriors (a later bgp_posterior_batch changes no bit of a path).  Needs d <= 32 and no context-level warp
 *   (BGP_ERR_INVALID), resident posteriors and every pidx among them (BGP_ERR_STATE).  Replaces an earlier state.
 * bgp_paths_eval: the P paths at m query rows: out P*m, dout P*m*d (may be NULL; the values are the same bits either way).  The
 *   value at (path, row) does not depend on which rows or paths share the call.  BGP_ERR_STATE without a state.
 * bgp_paths_end drops the state; bgp_ctx_update_data and bgp_ctx_destroy drop it too.
 * bgp_paths_stats: out[0] = begins, out[1] = evals run on this context.
 * bgp_chunk_stats: how the context's last call to an entry point that cuts its work by a scratch budget ran -- bgp_predict_batch /
 *   _warped / _gram, bgp_acq_batch, bgp_predict_mixture, bgp_sample_y_batch, bgp_knowledge_gradient, bgp_joint_entropy, bgp_grad_cov,
 *   bgp_predict_grad_batch, bgp_paths_eval, bgp_paths_minimize: out[0] = chunks of posteriors, out[1] = chunks of query rows,
 *   candidates or starts (per chunk of posteriors); a loop the entry point does not have counts as one chunk.  Host counters only.
 *   BGP_ITEM_CHUNK / BGP_ROW_CHUNK (below) force several chunks at small shapes (tests/test_gpu_chunk_loops.py).
 * bgp_paths_minimize: minimise every open path over the box [lo, hi] (d doubles each) from its OWN S starts,
 *   X0 P*S*d path-major, clipped into the box.  The objective is the path itself (normalised-y units).  ONE launch per chunk of
 *   starts, one workgroup per (start, path): a whole-workgroup evaluator of one path at one point (the identities above, every
 *   reduction in a fixed order, no atomics) drives the projected BFGS of bgp_minimize_starts -- the same device function -- with
 *   Armijo backtracking (at most max_iter iterations of at most 30 trial points).  Per (path, start), item p*S + s: X_out (inside
 *   the box exactly), f_out and g_out (P*S*d, may be NULL): the search's own evaluator at X_out; iters; evals (evaluations of the
 *   path, a closing one at X_out included where the last trial point was not X_out); status -- 0: the inf-norm of the projected
 *   gradient is <= gtol, 1: max_iter reached, 2: the line search found no decrease (or a non-finite iterate).  max_iter = 0 is a
 *   pure evaluation of the clipped starts (iters 0, evals 1).  A (path, start) result does not depend on what shares the call.
 *   S >= 1, max_iter >= 0, gtol >= 0 (BGP_ERR_INVALID); BGP_ERR_STATE without a state.  Does not read the resident posteriors.
 *   The staged outputs are chunked over S under the 2^24-double budget of bgp_paths_eval.
 *   Replaces: the argmin over 500 random rows of a joint draw in Optimizer.optimum_intervals (bask/optimizer.py:622-689).
 */
int bgp_paths_begin(bgp_ctx* ctx, int P, const int* pidx, const double* h_kernel, const double* s2, int F,
                    const double* omega, const double* phase, const double* w, const double* eps);
int bgp_paths_eval(bgp_ctx* ctx, int m, const double* Xq, double* out, double* dout);
int bgp_paths_end(bgp_ctx* ctx);
int bgp_paths_stats(bgp_ctx* ctx, long long* out2);
int bgp_chunk_stats(bgp_ctx* ctx, long long* out2);
int bgp_paths_minimize(bgp_ctx* ctx, int S, const double* X0, const double* lo, const double* hi, double gtol, int max_iter,
                       double* X_out, double* f_out, double* g_out, int* iters, int* evals, int* status);

/*
 * Joint batch selection on the open paths (csrc/bgp_paths_select.hip): q candidates picked greedily on the
 * joint draw of the P paths over {training inputs, candidates}, instead of one fantasy "lie" per point (bgp_fantasy_*).  Serves
 * Optimizer.ask(n_points > 1) (bask/optimizer.py:177-226, where the reference has no batch at all) with strategy "joint_ei" /
 * "thompson", and gives the Thompson draws of evaluate_acquisitions (bask/acquisition.py:132-136) a batch form.
 * The P paths are evaluated at the m candidates Xcand (m*d, row-major) into a device matrix F[s, i] by the launches of
 * bgp_paths_eval (the same bits), normalised-y units.  Incumbent of path s, c_s: incumbent = 0: the scalar y_opt; incumbent = 1: the
 * path's own minimum over the n training inputs (the same evaluator on the state's copy of them; min is exact): the incumbent of
 * "noisy EI", one per draw of function AND hyper-parameters.  inc_out (P, may be NULL) receives these c_s, before any candidate lowers
 * them.  Then the n_forced candidates forced[k] (points under evaluation; each index once) are applied in order: c_s = min(c_s,
 * F[s, forced[k]]), candidate marked chosen.  Then q greedy steps, j = 0 .. q - 1, without host synchronisation in between:
 *   kind = BGP_SELECT_IMPROVEMENT:  a_j(i) = (sum over s = 0 .. P - 1, ASCENDING, of max(0, c_s - F[s, i])) / P
 *       -- rounded differences, added one by one to a running sum that starts at 0, one division at the end, no contraction: the
 *       order is part of the contract, the same for every m, q and P (no chunking).  pick_j = the unchosen i of largest a_j(i), ties
 *       to the lowest index (np.argmax's order, bgp_fantasy_step's); then c_s = min(c_s, F[s, pick_j]).  a_j(i) is the gain of the
 *       Monte-Carlo q-EI  mean_s max(0, inc_s - min_{k in chosen} F[s, k])  when i joins the chosen set; a chosen candidate, or a row
 *       equal to one, has value exactly 0 at every later step, and a candidate's values never increase from step to step.
 *   kind = BGP_SELECT_THOMPSON:     a_j(i) = -F[j mod P, i];  pick_j = the unchosen argmax, same tie rule; c is not used (inc_out
 *       is still written).
 * picks: q indices.  values: q*m (may be NULL), row j = a_j over ALL candidates, chosen ones included.  a_j(i) depends on column i
 * of F and on c alone: not on the other candidates, nor on m.  Picks, values and incumbents come back in one transfer at the end.
 * F lives in one owned allocation for the duration of the call: P * mpad doubles, mpad = m rounded up to 256, at most
 * BGP_SELECT_MAX_DOUBLES (1 GiB) -- BGP_ERR_INVALID beyond, checked before anything is read.  BGP_ERR_INVALID also for: kind or
 * incumbent out of range, m < 1, q < 1, n_forced < 0, q + n_forced > m, a forced index outside [0, m) or repeated, a non-finite y_opt
 * with incumbent = 0.  BGP_ERR_STATE without a paths state.  Neither the paths state nor the resident posteriors are modified.
 */
#define BGP_SELECT_IMPROVEMENT 0
#define BGP_SELECT_THOMPSON 1
#define BGP_SELECT_MAX_DOUBLES ((size_t)1 << 27)
int bgp_paths_select(bgp_ctx* ctx, int m, const double* Xcand, int kind, int incumbent, double y_opt, int n_forced,
                     const int* forced, int q, int* picks, double* values, double* inc_out);

/*
 * Partial dependence of the surrogate mean on one or two input dimensions: the data of the "plot objective"
 * figure, for the resident posteriors 0 .. B-1 (h_kernel B*(d + 2) as in bgp_predict_batch; the white level is not read: cross
 * values carry none).  With S sample rows Xs (S*d) and a panel D = {k1} or {k1, k2} with grid values g (normalised-y units):
 *   pd_b(D, g) = (1 / S) sum_s sum_j alpha_bj k_b(x_s[D <- g], X_j)
 * evaluated from Q_sj = sum_{k not in D} (x_sk / l_k - X_jk / l_k)^2 and T_j(g) = sum_{k in D} (g_k / l_k - X_jk / l_k)^2 (both sums of
 * squares, ascending dimension), k = k(Q + T): the mean of bgp_predict_batch on the S synthesised rows of every cell to the
 * precision model's tolerance, not its bits.
 * grid is gmax*d row-major: column k holds dimension k's grid in its first ng[k] rows (the rest is not read); samples and grid rows
 * go through the context-level warp as predict's queries do.  panels is P*2 ints: (k1, -1) or (k1, k2), k1 != k2, either order,
 * repeats allowed.  out is B*total: panel p's block starts at the sum of the earlier panels' sizes and holds ng[k1] values, or
 * ng[k1]*ng[k2] row-major with k1's index slow.  A panel's values do not depend on which panels or posteriors share the call, nor
 * on its place in the list.
 * Needs d <= 32, S >= 1 (at most 65535*16), P >= 1, 1 <= ng[k] <= gmax <= 256, panel indices in [0, d), at most 2^30 cells
 * (BGP_ERR_INVALID before anything is launched) and B resident posteriors (BGP_ERR_STATE).
 *   Replaces: the per-cell predict loop of skopt.plots.partial_dependence (reached from bask's plot_objective).
 */
int bgp_partial_dependence(bgp_ctx* ctx, int B, const double* h_kernel, int S, const double* Xs, int gmax, const int* ng,
                           const double* grid, int P, const int* panels, double* out);

/*
 * Variance-based (Sobol') sensitivity of the surrogate mean by the pick-freeze design (csrc/bgp_sobol.hip),
 * for the resident posteriors 0 .. B-1 (h_kernel B*(d + 2) as in bgp_predict_batch; the white level is not read).  With two
 * sample matrices A, Bm (N*d each, row-major) and T terms, term t the set of dimensions whose bits are set in masks[t]:
 *   fA_i = mu_b(A_i),  fB_i = mu_b(Bm_i),  fT_ti = mu_b(A_i with the columns in masks[t] taken from Bm_i)    (normalised-y units)
 *   f0_b = (1 / 2N) sum_i (fA_i + fB_i)                 V_b     = (1 / 2N) sum_i ((fA_i - f0)^2 + (fB_i - f0)^2)
 *   closed_bt = (1 / N) sum_i (fB_i - f0) (fT_ti - fA_i)     total_bt = (1 / 2N) sum_i (fA_i - fT_ti)^2
 * (Saltelli et al. 2010 for the closed effect -- the first-order one for a single dimension --, Jansen 1999 for the total one; the
 * indices are closed / V and total / V, the caller's division.)  Every mean comes out of one routine applied to a synthetic row
 * whose squared distance to a training point is a sum of squares in x / l, ascending dimension: an empty mask gives fA and a full
 * one fB bit for bit (closed = total = 0 for the empty mask, and for every term when A == Bm).  The means (B*(T + 2)*N doubles of
 * device scratch) are reduced in a fixed order: chunks of 256 samples, a fixed tree inside a chunk, chunk partials in ascending
 * order, f0 before the centred sums.  f0, V and a term's closed / total depend on the posterior, A, Bm and that term alone: the same
 * bits whatever else shares the call, wherever the term stands in the list, whatever B is.  A and Bm go through the context-level
 * warp as predict's queries do.  f0, V: B;  closed, total: B*T, posterior-major.
 * Needs d <= 32, 1 <= N <= 2^24, 1 <= T <= 4096, 1 <= B <= 65535, B (T + 2) N <= 2^30, no mask bit at or above d (BGP_ERR_INVALID
 * before anything is launched) and B resident posteriors (BGP_ERR_STATE).
 *   Replaces: nothing in the reference -- there the route is predict on N (T + 2) synthesised rows and a reduction on the host.
 */
int bgp_sobol_indices(bgp_ctx* ctx, int B, const double* h_kernel, int N, const double* A, const double* Bm, int T,
                      const unsigned* masks, double* f0, double* V, double* closed, double* total);

/*
 * Posterior covariance of the surrogate's gradient, and the active-subspace sums (csrc/bgp_gcov.hip), for the
 * resident posteriors 0 .. B-1 (h_kernel B*(d + 2) as in bgp_predict_batch; the white level is not read: the latent function) at the m
 * query rows Xq (m*d, row-major).  With G_jk(x) = d k(x, X_j) / dx_k as in bgp_predict_grad_batch (cf = c in the product form, 1 in
 * the sum form; the constant and white terms add nothing) and phi = 1 (RBF), 3 (Matern 3/2), 5/3 (Matern 5/2):
 *   g(x)     = G(x)^T alpha                                   dmean  B*m*d        gradient of the mean
 *   Sigma(x) = diag(cf phi / l_k^2) - G(x)^T K^-1 G(x)        cov    B*m*d*d      posterior covariance of grad f(x)
 *   C_mean = (1 / m) sum_s g(x_s) g(x_s)^T,  C_cov = (1 / m) sum_s Sigma(x_s)      csum   B*2*d*d      C_mean, then C_cov
 * in normalised-y units per unit of the (transformed) input; K^-1 and alpha are the resident ones (alpha diagonal and noise as built).
 * Any output may be NULL, not all three.  Sigma is exactly symmetric (the lower triangle is computed and mirrored) and its diagonal
 * is clipped at 0 as bgp_predict_batch clips the variance.  The product G K^-1 runs on the fp64 MFMA ring; every sum has a fixed
 * order: a point's dmean and cov are the same bits whatever m and B are, whatever else shares the call and however the call is
 * chunked, and csum depends on the posterior and the ordered list of points alone (chunks of 256 points by their index in Xq, a
 * fixed tree inside a chunk, chunk partials in ascending order, one division by m).
 * Needs d <= 32, 1 <= m, m d <= 2^24, 1 <= B <= 65535, a family with a mean-square derivative -- Matern 1/2 is not differentiable
 * and is refused, never approximated -- and no context-level warp (warped inputs are refused as by the other gradient entry
 * points): BGP_ERR_INVALID before anything is launched; B resident posteriors: BGP_ERR_STATE.  A refused call leaves the resident
 * posteriors as they were.
 *   Replaces: nothing in the reference -- skopt's predict(return_std_grad) stops at the gradient of the std at one point.
 */
int bgp_grad_cov(bgp_ctx* ctx, int B, const double* h_kernel, int m, const double* Xq, double* dmean, double* cov, double* csum);

/*
 * Knowledge-gradient acquisition (csrc/bgp_kg.hip) of the resident posteriors 0 .. B-1 (h_kernel B*(d + 2) as
 * in bgp_acq_batch: the white level at -inf, the latent function) at the m candidates Xcand (m*d, row-major) against the M reference
 * points Xref (M*d; not read at M = 0).  noise (B): the variance of a fantasy observation per posterior, as bgp_fantasy_begin takes
 * it (constructor alpha + the row's white level).  In normalised-y units, for minimisation, with s = var_b(x) + noise_b and the
 * M + 1 lines  p_j = mu_b(a_j), q_j = cov_b(a_j, x) / sqrt(s)  (j < M),  p_M = mu_b(x), q_M = var_b(x) / sqrt(s)  (latent moments):
 *   KG_b(x) = min_j p_j - E_Z[min_j (p_j + q_j Z)],  Z ~ N(0, 1)      kg   B*m   y_std KG_b(x_i)
 *                                                                     avg  m     sum over b, ascending, of kg[b][i] / n_samples
 * clipped at 0, exactly 0 where s <= 0 and at M = 0.  A posterior whose values are not all finite contributes nothing to avg (the
 * rule of bgp_acq_batch).  Either output may be NULL, not both.  Lines of equal slope: the lower intercept wins; exact duplicates:
 * the lower index.  The product k_b(x, X) (K_b^-1 k_b(X, A)) runs on the fp64 MFMA ring; every sum has a fixed order: a candidate's
 * value is the same bits whatever m and B are, whatever else shares the call and however the call is chunked.
 * Needs d <= 32, 0 <= M <= 255, 1 <= m <= 2^24, 1 <= B <= 65535, 1 <= n_samples and no context-level warp: BGP_ERR_INVALID before
 * anything is launched; B resident posteriors that are not per-row warped: BGP_ERR_STATE.  A refused call leaves the resident
 * posteriors as they were; a successful one does not change them either.
 *   Replaces: nothing in the reference -- it has no acquisition that looks at the minimum of the posterior mean.
 */
int bgp_knowledge_gradient(bgp_ctx* ctx, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int M,
                           const double* Xref, double y_std, int n_samples, double* kg, double* avg);

/*
 * Joint entropy search acquisition (csrc/bgp_jes.hip) of the resident posteriors 0 .. B-1 (h_kernel B*(d + 2) as
 * in bgp_acq_batch: the white level at -inf, the latent function) at the m candidates Xcand (m*d, row-major).  Posterior b has its
 * OWN R samples of the optimum: locations Xopt (B*R*d, posterior-major) and values fopt (B*R).  noise (B): the variance of an
 * observation per posterior, as bgp_knowledge_gradient takes it (constructor alpha + the row's white level), > 0; tau >= 0: a
 * jitter on the noiseless optimum observation.  In normalised-y units, for minimisation, with latent moments mu, v of x and
 * mu_r, v_r of a_r, c_r = cov_b(a_r, x) = k_b(a_r, x) - k_b(a_r, X) K_b^-1 k_b(X, x) and w_r = v_r + tau:
 *   m_r = mu + c_r (f_r - mu_r) / w_r        v_s = max(v - c_r^2 / w_r, 0)         conditioning on f(a_r) = f_r
 *   z_r = (f_r - m_r) / sqrt(v_s)            v_t = clip(v_s F(z_r), 0, v_s)        f(x) >= f_r: lower truncation
 *   F(z) = 1 - lam (lam - z),  lam = phi(z) / Phi(-z)                              variance factor of a lower-truncated normal
 *   g_r = max(1/2 [log(v + noise_b) - log(v_t + noise_b)], 0)                      moment-matched entropy drop, nats
 *   gain  B*m   gain_b(x_i) = (1 / R) sum_r g_r           avg  m   sum over b, ascending, of gain[b][i] / n_samples
 * w_r <= 0: the sample conditions nothing (m_r = mu, v_s = v); v_s <= 0: v_t = 0.  A posterior whose values are not all finite
 * contributes nothing to avg (the rule of bgp_acq_batch).  Either output may be NULL, not both.  No y_std enters: nats.
 * F is a function of z alone: for z < 4 the definition with lam = sqrt(2 / pi) / erfcx(z / sqrt 2), from 4 on the Laplace continued
 * fraction lam = z + T, T = 1 / (z + U), U = 2 / (z + 3 / (z + ... 40 / z)), F = T (U - T), which has no cancellation.
 * Order of the sums: the two quotients 1 / w_r and (f_r - mu_r) / w_r are formed once per sample and multiplied by c_r^2 and c_r;
 * lane l of a 64-lane wave adds the terms r = l, l + 64, l + 128, l + 192 (< R) in that order, the lanes are added by the xor
 * butterfly 32, 16, 8, 4, 2, 1, then one division by R.  The product k_b(x, X) (K_b^-1 k_b(X, A_b)) runs on the fp64 MFMA ring.
 * A candidate's gain is the same bits whatever m and B are, whatever else shares the call, whichever outputs are asked for and
 * however the call is chunked.
 * Needs d <= 32, 1 <= R <= 255, 1 <= m <= 2^24, 1 <= B <= 65535, 1 <= n_samples, every noise[b] > 0 and finite, tau >= 0 and finite,
 * every fopt finite and no context-level warp: BGP_ERR_INVALID before anything is launched; B resident posteriors that are not
 * per-row warped: BGP_ERR_STATE.  A refused call leaves the resident posteriors as they were; a successful one does not change them
 * either.
 *   Replaces: nothing in the reference -- its only information-theoretic acquisition (mes) looks at the optimum's value alone.
 */
int bgp_joint_entropy(bgp_ctx* ctx, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int R,
                      const double* Xopt, const double* fopt, double tau, int n_samples, double* gain, double* avg);

/*
 * Cross-validation from the resident inverses (csrc/bgp_cv.hip): for each of the first B resident posteriors
 * and each fold F (fold f holds the training indices fold_idx[fold_ptr[f] .. fold_ptr[f + 1])), the predictive of the held-out
 * OBSERVATIONS y_F given all the other ones, without a refit.  With A = K^-1 (K with the alpha diagonal and the white level) and
 * a = A y, both resident after any posterior build:
 *   Sigma_F = (A_FF)^-1,  r_F = Sigma_F a_F,  mean_F = y_F - r_F,  var_i = (Sigma_F)_ii,
 *   fold_lpd = log N(y_F; mean_F, Sigma_F) = -1/2 a_F^T r_F + sum_k log C_kk - (|F| / 2) log 2 pi,   A_FF = C C^T.
 * One point per fold is the textbook leave-one-out: mean_i = y_i - a_i / A_ii, var_i = 1 / A_ii.  The variance is that of the
 * observation: the white level and the point's own alpha are in it (bgp_predict_batch's variance has neither alpha nor, with the
 * white level at -inf in h_kernel, the noise).  Everything is in the context's (normalised) y units.
 *   folds     disjoint index sets of [0, n), in any order, not necessarily contiguous, 1 .. 128 points each; they need not cover
 *             every point.  fold_ptr: n_folds + 1 ascending offsets from 0; fold_idx: fold_ptr[n_folds] indices.
 *   mean, var B*n, at the points' own positions; NaN where no fold covers the point.
 *   fold_lpd, status   B*n_folds.  status != 0: A_FF of that (posterior, fold) is not numerically positive definite (the 1-based
 *             failing pivot); its fold_lpd, mean and var are NaN and no other fold is affected.
 * Neither the training inputs nor the kernel are read, so plain, per-row-warped (bgp_posterior_batch_warped) and host-Gram
 * (bgp_posterior_batch_gram) posteriors are served alike.  A (posterior, fold) result depends on that posterior and that fold alone:
 * the same bits whatever B is and in whatever order the folds are listed.  When every fold is one point, one thread per
 * (posterior, point) reads the diagonal of the inverse; otherwise one workgroup per (posterior, fold) factorises A_FF in LDS sized
 * by the call's largest fold.
 * BGP_ERR_INVALID (before anything is launched, and before the residency answer): B < 1, an empty fold, a fold of more than 128
 * points (10-fold cross-validation beyond n = 1280), an index outside [0, n), an index listed twice.  BGP_ERR_STATE: fewer than B
 * resident posteriors, or a submitted batch pending.
 *   Replaces: nothing in the reference -- there the route is a refit per fold (theta setter on the remaining points + predict,
 *   bask/bayesgpr.py:200-217, 622-635).
 */
int bgp_cross_validate(bgp_ctx* ctx, int B, int n_folds, const int* fold_ptr, const int* fold_idx, double* mean, double* var,
                       double* fold_lpd, int* status);

/*
 * Draw f ~ N(mean, cov) at m points for resident posterior b using standard normals supplied by
 * the host (z: n_draws*m), via a Cholesky factor of cov (+jitter) instead of numpy's SVD.
 * Replaces: sklearn sample_y (sklearn/_gpr.py:522-526) reached from BayesGPR.sample_y
 * (bask/bayesgpr.py:637-718).  out: n_draws*m.  Returns BGP_ERR_NOTPD when cov + jitter*I is not
 * numerically positive definite (the caller retries with a larger jitter).
 */
int bgp_sample_y(bgp_ctx* ctx, int b, const double* h_kernel, int m, const double* Xq, int n_draws,
                 const double* z, double jitter, double* out);

/*
 * One draw per hyper-posterior sample, batched: item i draws f_i ~ N(mean_i, cov_i) at the m points from the
 * resident posterior pidx[i] with kernel parameters h_kernel[i] (B*(d+2)) and the standard normals z[i] (B*m);
 * out is B*m.  The B covariance matrices are factorised by ONE batched Cholesky.  status[i] != 0: cov_i + jitter*I
 * not numerically positive definite (out[i] undefined; the caller retries those items with a larger jitter).
 * Replaces: the per-sample loop of BayesGPR.sample_y(sample_mean=False) -- theta setter + sklearn sample_y per
 * chain row (bask/bayesgpr.py:679-718) -- after one bgp_posterior_batch over the drawn chain rows.
 */
int bgp_sample_y_batch(bgp_ctx* ctx, int B, const int* pidx, const double* h_kernel, int m, const double* Xq,
                       const double* z, double jitter, double* out, int* status);

/*
 * Generic kernel expression trees.  The reference accepts ANY skopt / scikit-learn kernel (bask/bayesgpr.py:148-159; priors by
 * recursion over arbitrary Sum / Product trees, bask/utils.py:154-179) and evaluates it on the host: K = kernel_(X_train)
 * (sklearn/_gpr.py:582).  For trees that have no canonical device form (two stationary terms, products of stationaries, general
 * Matern nu, RationalQuadratic, ...) the host side does exactly that with the scikit-learn kernel object and hands the matrices
 * over; the device does everything behind them -- diagonal add, factorisation, solves, log-likelihood, inverse, predictive
 * products: the same kernels as the canonical path, no factorisation on the host.
 *   K      B matrices of n*n doubles, row-major: kernel_(X_train) WITHOUT the alpha term; use_alpha != 0 adds the context's
 *          alpha_diag on the device (sklearn/_gpr.py:585)
 *   bgp_lml_batch_gram        as bgp_lml_batch        (sklearn/_gpr.py:537-613 via bask/bayesgpr.py:374)
 *   bgp_posterior_batch_gram  as bgp_posterior_batch  (bask/bayesgpr.py:200-217); the posteriors stay resident
 *   bgp_predict_batch_gram    as bgp_predict_batch for the B resident posteriors with host-evaluated cross covariances:
 *          Ks B*m*n = kernel_(Xq, X_train), kss B*m = kernel_.diag(Xq), Kss B*m*m = kernel_(Xq) (read only when cov != NULL)
 *          (bask/bayesgpr.py:622-635 -> skopt predict)
 */
int bgp_lml_batch_gram(bgp_ctx* ctx, int B, const double* K, int use_alpha, double* lml, int* status);
int bgp_posterior_batch_gram(bgp_ctx* ctx, int B, const double* K, int use_alpha, double* L, double* alpha, double* K_inv,
                             double* lml, int* status);
int bgp_predict_batch_gram(bgp_ctx* ctx, int B, int m, const double* Ks, const double* kss, const double* Kss, double* mean,
                           double* var, double* cov);

/* Number of walker groups (HIP streams) an LML batch of the launch schedule is split over; results are bit-identical for
 * every count.  Default: ONE group.  With k > 1 groups a batch of at least 64 matrices (or, after this call, of at least 16) is
 * factorised as k slices side by side, one group's kernels filling the tails of another's launches.  Two groups were the
 * default for batches of >= 64 matrices while that paid (+3.7 % at n = 2048 x 128 matrices on MI355X in round 2, nothing any
 * more in round 6); the fused panel launches (bgp_set_panel_fused) take whole CUs, and one group measured faster with them
 * (docs/EXPERIMENTS.md G29).  This call, or the environment variable BGP_STREAMS read at context creation, fixes the count.
 *
 * Environment switches the library reads (a BGP_* variable it does not read is reported once on stderr; the table of all of
 * them, with the moment each is read, is bgp_switches in csrc/bgp_plan.h and DESIGN.md section 19).  Schedule switches --
 * each selects between code paths whose results are bit-identical (tests/test_gpu_edge.py, tests/test_gpu_persist.py):
 *   BGP_STREAMS (this call), BGP_PANELS (block columns per trailing update, 1..64; default 4 from n = 1536, else 2), BGP_PERSIST
 *   (bgp_set_persist), BGP_PANEL_FUSED (bgp_set_panel_fused), BGP_PS_PAIR (0 / 1: one or two chain workgroups per matrix on the launch-free path; default by shape),
 *   BGP_PS_GEN (0 / 1: the Gram blocks of a launch-free LML batch are built by a kernel in front of it / by its own tile workers
 *   at the head of their ticket list; default by shape), BGP_SYRK_GEN (0 / 1: on the launch schedule, every Gram block by the
 *   kernel in front / all but block column 0 in the accumulators of the first panel group's updates; default 1 where the
 *   pipelined Gram kernel would run, see bgp_lml_gen_stats), BGP_GCOV_CHUNK (query points per chunk of bgp_grad_cov, rounded up to
 *   256; default by n and d; read at every call), BGP_KG_CHUNK / BGP_JES_CHUNK (candidates per chunk of bgp_knowledge_gradient / bgp_joint_entropy, rounded up to 128;
 *   default by n; read at every call), BGP_ITEM_CHUNK / BGP_ROW_CHUNK (upper bounds on the posteriors per chunk of the batched posterior
 *   calls and on the query rows / starts per chunk of bgp_predict_grad_batch, bgp_paths_eval and bgp_paths_minimize; default: the
 *   scratch budgets alone; read at every call; a bound can shrink a chunk, never enlarge it: see bgp_chunk_stats).
 * Runtime switch set by the PYTHON package, not read by this library: bayes-skopt_amd/_lib.py exports HIP_FORCE_DEV_KERNARG=1 (kernel
 *   arguments in device memory: -6 % per call on the launch schedule at n = 1024 x 32) at import unless the user has set it --
 *   a process-wide setting that every other HIP user of the process inherits, effective only if the GPU has not been initialised
 *   before the import; BGP_NO_ENV_DEFAULTS=1 leaves the environment alone.  A C caller of libbgp.so sets it itself.
 * Waits and diagnostics (no effect on results): BGP_WAIT=block, BGP_PS_TIMEOUT_MS, BGP_PS_COOLDOWN, BGP_PS_TRACE,
 *   BGP_COMM_TIMEOUT_S (DESIGN.md sections 2, 7 and 4).  The A/B switches of earlier rounds (BGP_FUSED_GRAM, BGP_KBUILD1,
 *   BGP_SMALL_SPLIT, BGP_PS_NCRIT / _PSPLIT / _STREAM, BGP_PANEL_WIDTH, BGP_ROWQUAD_T) left the library in round 5 with the
 *   measured-slower variants they selected. */
int bgp_set_streams(bgp_ctx* ctx, int nstreams);

/* hipDeviceSynchronize on `device` (timing brackets in bench.py). */
int bgp_device_synchronize(int device);

/* ---- measurement hooks (bench.py / profiling; not part of the reference surface) ---- */

/* Average device time (ms, HIP events on the context's stream) of the kernels of the last
 * bgp_lml_batch call: out[0]=K-build, out[1]=potrf (diagonal blocks), out[2]=trsm (panels),
 * out[3]=syrk (trailing update), out[4]=whole call on device; counts[0..3] = launches. */
int bgp_last_timing(bgp_ctx* ctx, double* out_ms, int* counts);
/* Time (ms) and count of the look-ahead column launches of the trailing update (K = 128 .. 128 (P-1), one block column)
 * inside out[3] of bgp_last_timing, for the last timed bgp_lml_batch call. */
int bgp_last_timing_columns(bgp_ctx* ctx, double* ms, int* launches);
/* Launch-free factorisation of small batches (one persistent kernel per bgp_lml_batch call -- and per covariance of
 * bgp_sample_y -- instead of ~3 launches per block column; same bits): 1 = whenever the batch fits (<= 64 matrices,
 * n > 128), 0 = never, -1 = as BGP_PERSIST says (unset: where it measured faster on MI355X: at least 6 block columns of
 * 128, matrices x block columns <= 400; and -- with two chain workgroups per matrix -- few matrices from 3 block columns on:
 * bgp_persist_auto_rule / bgp_pair_auto_rule in csrc/bgp_plan.h).  Replaces nothing in the reference; a scheduling choice behind cholesky() of
 * sklearn/_gpr.py:587. */
int bgp_set_persist(bgp_ctx* ctx, int mode);
/* Bookkeeping of that path: out[0] = launch-free calls enqueued by this context, out[1] = of which timed out (a wait
 * outlasted BGP_PS_TIMEOUT_MS, 500 ms: the workgroups were not co-resident; the batch was redone by launches, same
 * results), out[2] = 1 while a time-out keeps the path switched off, out[3] = eligible calls left before it is tried again
 * (BGP_PS_COOLDOWN, 256; after the third time-out the path stays off until bgp_set_persist(ctx, 1)).  A context that shares
 * its device with other contexts, processes or collectives should call bgp_set_persist(ctx, 0). */
int bgp_persist_stats(bgp_ctx* ctx, long long* out4);
/* Gram generation inside the trailing update (launch schedule of the LML path; csrc/bgp_s4.h S4GenF): the kernel matrix K(X, X) of
 * sklearn/_gpr.py:582-585 is built by the Gram kernel for block column 0 only; every other block is computed in the accumulators
 * of the update of the first panel group that touches it first (same arithmetic per element: same bits; BGP_SYRK_GEN=0 builds every
 * block with the Gram kernel in front).  out[0] = LML batches (per walker-group stream) factorised that way by this context,
 * out[1] = generating launches among their trailing updates. */
int bgp_lml_gen_stats(bgp_ctx* ctx, long long* out2);
/* Launch schedule, LML path: the diagonal factorisation and the panel solve of a block column in ONE launch (panel_kernel,
 * csrc/bgp_chol.hip: the inverse W_kk of the diagonal factor stays in LDS, and CUs that idle during a separate potrf launch
 * factorise the block redundantly and share the solve; same bits as potrf_kernel + trsm4_kernel): 1 = every block column that has
 * a solve, 0 = never, -1 = as BGP_PANEL_FUSED says (unset: where it measured faster on MI355X, bgp_panel_fused_rule).  A scheduling
 * choice behind cholesky() / cho_solve() of sklearn/_gpr.py:587-597.  With timing on, a fused launch counts under "trsm", which is
 * then the panel phase of those block columns. */
int bgp_set_panel_fused(bgp_ctx* ctx, int mode);
/* out[0] = fused panel launches enqueued by this context. */
int bgp_panel_fused_stats(bgp_ctx* ctx, long long* out1);
/* Enable (1) / disable (0) per-kernel event timing (adds synchronisation; off by default). */
int bgp_set_timing(bgp_ctx* ctx, int enable);
/* Debugging aid (BGP_PS_TRACE=1): in-kernel wall-clock stamps (100 MHz) of the last launch-free call.  dims = {matrices,
 * block columns, tile tasks}; out (may be NULL to query dims) receives 8 stamps per (matrix, block column) of the chain
 * role, then 8 per tile task; cap = capacity of out in 64-bit words.  Read by tools/persist_trace.py. */
int bgp_debug_ps_trace(bgp_ctx* ctx, int* dims, unsigned long long* out, size_t cap);
/* What the library would launch for one LML batch of nb matrices (one chunk: nb <= max_batch), from the launch planner alone
 * (csrc/bgp_plan.h; DESIGN.md sections 3, 4 and 19): nothing is enqueued, counted or changed.  With a context, the shape, the
 * device and the modes are the context's and the query supplies nb and warped; the launch-free path counts as permitted unless a
 * time-out or an open resident sampler redo keeps it off right now.  With ctx == NULL the query is complete and no device is
 * touched (a machine without a GPU answers).  Either way the live switches (BGP_SYRK_GEN, BGP_PS_PAIR, BGP_PS_GEN) are the
 * environment's, read as an LML call reads them. */
typedef struct bgp_lml_plan_query {
  int nb, warped;
  /* ctx == NULL only: */
  int n, d, stationary, form; /* rows, input dimensions, BGP_RBF .., BGP_FORM_.. */
  int ncu;                    /* compute units of the device */
  int timing, persist, panel_fused; /* bgp_set_timing; bgp_set_persist, bgp_set_panel_fused: -1 by shape, 0, 1 */
  int panels, nstreams;       /* BGP_PANELS, bgp_set_streams; 0: the default */
  int ps_permitted;           /* no time-out keeps the launch-free path off */
} bgp_lml_plan_query;
#define BGP_PLAN_REPORT_COLS 256
typedef struct bgp_lml_plan_report {
  int nblk, ncu, fits;  /* block columns of 128, CUs planned for, the batch could take the launch-free path at all */
  int path;             /* 0: n <= 128, one fused launch; 1: launch-free; 2: launch schedule */
  /* launch schedule: `share` walker-group streams share the CUs; ngroups groups of gsz matrices (the last: nb_last); P block
   * columns per trailing update; Gram blocks generated inside the trailing update by the first / the last group / by how many */
  int share, gsz, ngroups, nb_last, P, gen_first, gen_last, gen_groups;
  /* launch-free path: PsArgs of csrc/bgp_common.h, the tile workgroups, and whether the Gram kernel goes in front */
  int pair, Bpad, nchain, psplit, dsplit, ncrit_stream, ncrit, ps_gen, total, tile_wgs, gram_front;
  /* launches the plan enqueues, by the categories of bgp_last_timing (a fused panel launch under trsm, a look-ahead column
   * under syrk too), the fused and the generating ones among them, and the launch-free kernel */
  int kbuild, potrf, trsm, syrk, columns, fused, generating, launch_free;
  /* launch schedule: workgroups per matrix of the fused launch of block column k in the first / the last group, 0: separate
   * potrf + trsm launches (the first BGP_PLAN_REPORT_COLS block columns) */
  int fused_wgs[BGP_PLAN_REPORT_COLS], fused_wgs_last[BGP_PLAN_REPORT_COLS];
} bgp_lml_plan_report;
int bgp_debug_lml_plan(bgp_ctx* ctx, const bgp_lml_plan_query* query, bgp_lml_plan_report* report);
/* Debugging aid: working matrix (npad x npad doubles; L in the lower triangle after an LML call) and working right-hand
 * side (npad doubles, z = L^-1 y) of batch slot b as the last bgp_lml_batch left them; either pointer may be NULL. */
int bgp_debug_workspace(bgp_ctx* ctx, int b, double* L, double* z);
/* Debugging aid: the Cholesky factor of the predictive covariance as the last bgp_sample_y left it (*mpad = its padded
 * edge, a multiple of 128, 0 when there is none; L: mpad x mpad doubles, lower triangle; may be NULL to query mpad). */
int bgp_debug_cov_factor(bgp_ctx* ctx, int* mpad, double* L);
/* Debugging aid / accuracy test: sqrt(x[i]) and 1 / sqrt(x[i]) as the diagonal-block factorisation forms its pivots
 * (hardware seed + coupled Goldschmidt step + one residual correction each; LAPACK dpotrf's sqrt via sklearn/_gpr.py:587). */
int bgp_debug_pivot_root(int device, int n, const double* x, double* sqrt_out, double* rsqrt_out);
/* fp64 MFMA micro-benchmark: TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64 on the whole chip. */
int bgp_bench_mfma_f64(int device, int iters, double* tflops);
/* HBM copy micro-benchmark: GB/s (read+write) of a streaming double2 copy of `bytes` bytes. */
int bgp_bench_hbm_copy(int device, long long bytes, int iters, double* gbps);
/* Empirical C/D fragment layout of v_mfma_f64_16x16x4_f64: rows[64*4], cols[64*4] (lane*4+reg). */
int bgp_mfma_f64_layout(int device, int* rows, int* cols);

/*
 * Multi-GPU exchange over RCCL (one process per GPU).  The hot path shards by chains: no collective in
 * the sampling loop, ONE all-gather of the posterior samples at the end (bgp_comm_allgather; in the exact
 * single-ensemble option also the B log-probabilities of each half-step).  Host buffers in, host buffers out; the
 * staging buffers stay resident on the device.  bgp_comm_unique_id is called on rank 0 and its BGP_COMM_ID_BYTES bytes
 * are handed to every rank by the caller (bayes-skopt_amd/distributed.py: a per-job file in a per-user directory on a
 * single node, a TCP socket on MASTER_ADDR:(MASTER_PORT + 1) across nodes).
 * Replaces: nothing in the reference (it is single-process); mirrors what torch.distributed's all_gather /
 * all_reduce(MAX) / broadcast would do, without PyTorch in the product path.
 */
#define BGP_COMM_ID_BYTES 128
typedef struct bgp_comm bgp_comm;
int bgp_comm_available(void); /* 1 when librccl.so can be loaded in this process */
int bgp_comm_unique_id(void* id128);
int bgp_comm_init(int device, int rank, int world, const void* id128, bgp_comm** out);
void bgp_comm_destroy(bgp_comm* comm);
/* recv (world * count doubles) = concatenation of every rank's send (count doubles), rank-major */
int bgp_comm_allgather(bgp_comm* comm, const double* send, size_t count, double* recv);
int bgp_comm_allreduce_max(bgp_comm* comm, double* inout, size_t count);
int bgp_comm_broadcast(bgp_comm* comm, double* buf, size_t count, int root);
int bgp_comm_barrier(bgp_comm* comm);
/* This rank is going down outside a collective (interrupt, fatal error): ncclCommAbort, so that the peers' collectives fail at
 * once (BGP_ERR_COMM on their side) instead of waiting BGP_COMM_TIMEOUT_S; every later call on the communicator answers BGP_ERR_COMM. */
int bgp_comm_abort(bgp_comm* comm);
/* ranks RCCL counts in the communicator (ncclCommCount) */
int bgp_comm_nranks(bgp_comm* comm, int* nranks);
/* Loop-back communicator: rank `rank` of a group of `world` communicators of THIS process on ONE device (one per host thread, each
 * beside its own context; the communicators that name the same key form the group).  It serves the in-stream exchange of a
 * sharded bgp_mcmc_begin_ex run with device copies and events instead of RCCL -- the row-sharding logic of the multi-GPU sampler
 * exercised with world > 1 semantics on a single GPU (tests); every other collective answers BGP_ERR_COMM. */
int bgp_comm_init_loopback(int device, int rank, int world, long long key, bgp_comm** out);
/* Measurement hook (bench.py): `reps` rounds of the sharded resident sampler's per-half-step exchange (pack kernel + all-gather of
 * per + 1 doubles per rank) back to back on the CONTEXT's stream between two HIP events: the device-side price of the exchange
 * where the sampler pays it, ms per round.  Every rank of the communicator calls it together. */
int bgp_comm_bench_lml_gather(bgp_ctx* ctx, bgp_comm* comm, int per, int reps, double* ms_per_round);
/* Exact single-ensemble sharding of bask/bayesgpr.py:490-530 (ONE n_walkers ensemble, one RNG): every rank has
 * submitted its own rows of a half-step's proposal block with bgp_lml_batch_submit (possibly none); this replaces
 * bgp_lml_batch_wait and returns the log-likelihoods of ALL ranks (world * per_rank doubles, rank-major, gathered device to
 * device out of every context's resident result vector: the communicator's stream waits for the context's stream through
 * an event, ONE host synchronisation per half-step).
 * Every rank must ENTER this call once it has been agreed on (RCCL has no time-out): a rank whose own work failed between
 * submit and wait passes local_error > 0 instead of returning early; its values travel as NaN and errors_out[r] (world
 * ints, identical on every rank) carries the code, so that all ranks raise alike.  A rank whose launch-free factorisation
 * timed out redoes its batch by launches and all ranks repeat the gather (decided from the same gathered status word).
 * The pending batch is consumed whatever the outcome.  Returns BGP_OK when the collective completed (inspect errors_out),
 * BGP_ERR_COMM when it did not within BGP_COMM_TIMEOUT_S seconds (default 300) or RCCL reported an asynchronous error:
 * the communicator is aborted (ncclCommAbort) and every later collective on it answers BGP_ERR_COMM. */
int bgp_lml_batch_wait_allgather(bgp_ctx* ctx, bgp_comm* comm, int per_rank, int local_error, double* lml_all,
                                 int* errors_out);

/* ---- the ensemble sampler with its state resident in HBM ------------------------------------------------------------
 * Replaces the per-half-step traffic of emcee's loop (bask/bayesgpr.py:510-530 -> emcee 3.1.6 EnsembleSampler.sample with
 * one StretchMove: propose, compute_log_prob, accept, for each half of the ensemble): nsteps steps of W walkers (W even) with p
 * entries each run on the device without a transfer or a synchronisation in between.  The caller draws every random number of
 * the run in emcee's stream order (none depends on a log-probability) and passes them as the plan, 2 * nsteps half-steps of
 * Ns = W / 2 rows: movers / partners (walker indices), zz (the stretch factors z), factors ((p - 1) log z) and logu (log of
 * the accept draws).  A proposal is q = c - (c - s) z (s = coords[mover], c = coords[partner]); its canonical hyper-parameters
 * are h[j] = h_src[j] >= 0 ? q[h_src[j]] : h_fixed[j] (j < d + 2); its log-prior is the sum over the p entries, in order, of
 *   prior_kind 1:  par[0] - 0.5 exp(t) / par[1] + 0.5 t                      (half-Normal on sqrt(exp t), bask/utils.py:95-99)
 *   prior_kind 2:  (-2 (exp(par[2] (t - par[0])) + exp(par[3] (t - par[1]))) - par[4]) + t   (round-flat on exp t, bask/priors.py:7-57:
 *                  -2 ((x / lo)^p_lo + (x / hi)^p_hi) - log_norm with par = (ln lo, ln hi, p_lo, p_hi, log_norm))
 * (prior_par: p x 5); log-probability = log-prior + LML, non-finite -> -inf (bask/bayesgpr.py:351-379); accept iff
 * factors + lp_new - lp_old > logu.  Outputs: chain (nsteps x W x p) and logp (nsteps x W) after every step, the final
 * ensemble (coords_out, logp_out), accept counts, and info (4 ints): info[0] != 0 when a proposal had a non-finite coordinate
 * (emcee raises ValueError there: the caller should) -- info[2] is then the index of the first such half-step and info[3] says
 * whether its first offender was a NaN (1) or an infinity (0), as emcee's two messages distinguish --, info[1] = 1 when a
 * launch-free factorisation gave up its waits and the WHOLE run was redone on the launch schedule (same bits).  Needs the rows of a
 * half-step that this context factorises (W / 2, or its share of them) <= max_batch, no pending batch, per-launch timing off.  An
 * ensemble too large for the step kernel's 160 KB of LDS (W p + W + 3 Ns + 2 Ns p > 20 480 doubles) runs the same kernel on the
 * arrays in HBM; n <= 128 with at most 64 entries per walker takes the fused one-launch half-step.
 * bgp_mcmc_begin / bgp_mcmc_steps / bgp_mcmc_end are the same run with the plan handed over in segments (nseg steps = 2 nseg rows
 * of every plan array per call, in order): bgp_mcmc_steps uploads its rows, enqueues their half-steps and returns at once, so the
 * caller draws the next segment's random numbers while the device works through this one; bgp_mcmc_end (every step handed over)
 * waits and collects.  Between begin and end the context belongs to the run: every other entry point answers BGP_ERR_STATE;
 * bgp_ctx_destroy drops an open run.  bgp_mcmc_run = begin + one bgp_mcmc_steps with the whole plan + end.
 * bgp_mcmc_progress: steps of the open run whose segment the device has worked through (never blocks): what a progress bar shows
 * while the run is resident (emcee's tqdm bar, bask/bayesgpr.py:522-524 with progress=True, the default of fit, :550-564).
 * bgp_mcmc_form (debugging aid): the form of the half-step the open run takes -- 0 the step kernel with the ensemble in LDS, 1 the
 * step kernel on the arrays in HBM, 2 the fused one-launch half-step.
 *
 * bgp_mcmc_begin_ex adds the two things that change the SHAPE of a half-step:
 *   nwarp = 2 d   walkers that carry their own input warp (warp_inputs=True, bask/bayesgpr.py:353-365): the last 2 d entries of a
 *                 walker are [wa_1 .. wa_d, wb_1 .. wb_d] (log space) and every proposal's Gram matrix is built on the design
 *                 matrix seen through the Beta CDFs of ITS parameters (the kernels of bgp_lml_batch_warped); h_src only reads the
 *                 first p - 2 d entries.  Log-prior = sum over those entries, in order, + sum over k of (prior(wa_k) + prior(wb_k))
 *                 (the reference's two loops, :360-372).  prior_kind 3:  ((-(y y)) / 2 - par[2]) - par[3], y = (t - par[0]) / par[1]
 *                 (Normal(loc, scale) on t with par = (loc, scale, log sqrt(2 pi), log scale): scipy's norm.logpdf operation by
 *                 operation, the default warp priors of bask/bayesgpr.py:463-466).  0: no warp.
 *   comm          ONE ensemble sharded over the ranks of a communicator (SURVEY.md 8e option 1): every rank calls with the same
 *                 arguments and the same plan; the step kernel runs replicated on every rank, rank r factorises rows
 *                 [r Ns / G, (r + 1) Ns / G) of every half-step's proposal block, and an all-gather of ceil(Ns / G) + 1 doubles per
 *                 rank (log-likelihoods + a status word) sits between the LML batch and the next step kernel ON THE CONTEXT'S
 *                 STREAM -- no host synchronisation per half-step, the chain equals the one-GPU chain bit for bit.  A rank whose
 *                 launch-free factorisation timed out says so in its status word and EVERY rank redoes the whole run on the launch
 *                 schedule; bgp_mcmc_end waits with the communicator's bound (BGP_COMM_TIMEOUT_S) and returns BGP_ERR_COMM instead
 *                 of hanging; a rank that drops its run early aborts the communicator.  NULL: one rank. */
int bgp_mcmc_begin_ex(bgp_ctx* ctx, bgp_comm* comm, int nwarp, int W, int p, int nsteps, const int* h_src,
                      const double* h_fixed, const int* prior_kind, const double* prior_par, const double* coords0,
                      const double* logp0);
int bgp_mcmc_progress(bgp_ctx* ctx, int* steps_done);
int bgp_mcmc_form(bgp_ctx* ctx, int* form);
int bgp_mcmc_begin(bgp_ctx* ctx, int W, int p, int nsteps, const int* h_src, const double* h_fixed, const int* prior_kind,
                   const double* prior_par, const double* coords0, const double* logp0);
int bgp_mcmc_steps(bgp_ctx* ctx, int nseg, const int* movers, const int* partners, const double* zz, const double* factors,
                   const double* logu);
int bgp_mcmc_end(bgp_ctx* ctx, double* chain, double* logp, double* coords_out, double* logp_out, long long* naccepted, int* info);
int bgp_mcmc_run(bgp_ctx* ctx, int W, int p, int nsteps, const int* h_src, const double* h_fixed, const int* prior_kind,
                 const double* prior_par, const double* coords0, const double* logp0, const int* movers, const int* partners,
                 const double* zz, const double* factors, const double* logu, double* chain, double* logp, double* coords_out,
                 double* logp_out, long long* naccepted, int* info);

#ifdef __cplusplus
}
#endif
#endif /* BGP_H */
