/*
 * smcnuts_hip.h -- C ABI of libsmcnuts_hip.so: the MI355X (gfx950) hot path of
 * SMC-NUTS behind the reference's own operator boundary.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to UoL-SignalProcessingGroup/SMC-NUTS @ 2024_10_08).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; smcn_last_error()
 *     gives the message (owned by the library, valid until the next call on
 *     that context, or on a NULL context: until the next failing create);
 *   - the caller owns every host buffer; the library owns device memory;
 *   - host matrices are row-major [N, D] fp64 exactly as the reference's NumPy
 *     arrays; on the device the particle state is kept [D, N] ("dim-major")
 *     so that lane-adjacent particles are address-adjacent;
 *   - one context = one GPU = one shard of N particles; not re-entrant;
 *   - all calls are synchronous on return unless the name ends in _async.
 */
#ifndef SMCNUTS_HIP_H
#define SMCNUTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smcn_ctx smcn_ctx;

/* Device-native targets (replace smcnuts/model/bridgestan.py:7-146, whose
 * BridgeStan back end cannot be called from device code). */
#define SMCN_MODEL_GAUSS 0  /* data = [D, prior_sd, has_lik, lik_mean, lik_sd]            */
#define SMCN_MODEL_ARMA 1   /* data = [T, y_1..y_T]                 stan_models/arma/arma.stan   */
#define SMCN_MODEL_PRMWCD 2 /* data = [N, M, Clength, q, y.., Xkernel..]  stan_models/PRMwCD/PRMwCD.stan */
#define SMCN_MODEL_HOST 3   /* data = [D]: the density is the caller's (smcn_set_host_target)              */
#define SMCN_MODEL_GLM 4    /* data = [family (0 bernoulli_logit, 1 poisson_log), n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)], D = p + intercept <= 64;
                              family 2 (normal, sigma = e^tau) or 3 (neg_binomial_2_log, phi = e^tau): [family, n, p, intercept,
                              s_1..s_Dc, m_tau, s_tau, y_1..y_n, X], Dc = p + intercept, x = (b_1..b_Dc, tau), D = Dc + 1 <= 64,
                              tau ~ N(m_tau, s_tau^2); constrain reports e^tau */
#define SMCN_MODEL_HGLM 5   /* varying-intercept GLM, non-centred: data = [family (0..3 as SMCN_MODEL_GLM), n, p, intercept, J,
                              s_1..s_Dc, s_tau, (m_d, s_d: families 2, 3), y_1..y_n, g_1..g_n (in 0..J-1), X (n x p, row-major)],
                              Dc = p + intercept >= 0, J >= 1 groups; eta_i = [b_0 +] X_i b + e^lt z_{g_i}, b_c ~ N(0, s_c^2),
                              z_j ~ N(0, 1), e^lt ~ half-normal(s_tau), ld ~ N(m_d, s_d^2) (dispersion e^ld);
                              x = (b_1..b_Dc, z_1..z_J, lt [, ld]), D = Dc + J + 1 (+ 1) <= 64;
                              constrain reports (b, e^lt z_1..e^lt z_J, e^lt [, e^ld]) */
#define SMCN_MODEL_CATEGORICAL 6   /* categorical (multinomial logistic) regression, class 0 the reference: data = [K, n, p,
                              intercept, s_1..s_D, y_1..y_n (labels in 0..K-1), X (n x p, row-major)], 2 <= K <= 16,
                              Dc = p + intercept >= 1; eta_i0 = 0, eta_ik = [b_k0 +] X_i b_k (k = 1..K-1),
                              log p(y_i) = eta_{i,y_i} - logsumexp_k eta_ik, b_c ~ N(0, s_c^2);
                              x = (b_1,1..b_1,Dc, .., b_K-1,1..b_K-1,Dc) class-major, D = (K - 1) Dc <= 64;
                              constrain is the identity */
#define SMCN_MODEL_ORDINAL 7   /* ordinal (ordered-logistic) regression, no intercept: data = [K, n, p, s_1..s_p, t_1..t_{K-1},
                              y_1..y_n (labels in 0..K-1), X (n x p, row-major)], K >= 2, p >= 0; eta_i = X_i b,
                              cutpoints c_1 = u_1, c_k = c_{k-1} + e^u_k, P(y_i = k) = logit^-1(eta_i - c_k) -
                              logit^-1(eta_i - c_{k+1}) (c_0 = -inf, c_K = +inf), b_j ~ N(0, s_j^2), c_k ~ N(0, t_k^2) with
                              the log-Jacobian sum_{k>=2} u_k; x = (b_1..b_p, u_1..u_{K-1}), D = p + K - 1 <= 64;
                              constrain reports (b, c_1..c_{K-1}) */
#define SMCN_MODEL_MLGLM 8   /* multilevel GLM, non-centred, R independent varying terms (slopes, crossed factors): data =
                              [family (0..3 as SMCN_MODEL_GLM), n, p, intercept, R, J_1, J_2, J_3, J_4 (0 beyond R),
                              s_1..s_Dc, s_tau_1..s_tau_R, (m_d, s_d: families 2, 3), y_1..y_n, then for each term r = 1..R
                              g_r1..g_rn (in 0..J_r-1) and z_r1..z_rn (finite; 1 = varying intercept, a covariate = varying
                              slope), X (n x p, row-major)], 1 <= R <= 4, J_r >= 1, Dc = p + intercept >= 0;
                              eta_i = [b_0 +] X_i b + sum_r z_ri e^lt_r u_{r,g_ri}, b_c ~ N(0, s_c^2), u_rj ~ N(0, 1),
                              e^lt_r ~ half-normal(s_tau_r), ld ~ N(m_d, s_d^2) (dispersion e^ld);
                              x = (b_1..b_Dc, u_1,1..u_1,J1, .., u_R,1..u_R,JR, lt_1..lt_R [, ld]),
                              D = Dc + sum_r J_r + R (+ 1) <= 64;
                              constrain reports (b, e^lt_r u_rj .., e^lt_1..e^lt_R [, e^ld]) */
#define SMCN_MODEL_WGLM 9    /* wide GLM: SMCN_MODEL_GLM's model and data block, word for word (families 0..3, the same priors,
                              the same constrained space (b [, e^tau])), for 65 <= D <= 256 coordinates (D = p + intercept, + 1
                              for tau in families 2 and 3).  D <= 64 is refused (SMCN_MODEL_GLM), D > 256 runs host-evaluated.
                              Sampling, moments, summaries and shards as for any device model; the pointwise criteria,
                              PSIS-LOO, prediction and predictive draws keep a row in registers and stay with
                              SMCN_MODEL_GLM; smcn_gauss_lkernel_sums refuses D > 64 as for every model */
#define SMCN_MODEL_OGLM 10   /* GLM with per-observation offsets and / or weights: SMCN_MODEL_GLM's families 0..3, priors,
                              coordinates and constrained space (b [, e^tau]), D <= 64, with
                                eta_i = [b_0 +] X_i b + o_i,   llik = sum_i w_i l(y_i | eta_i [, tau]);
                              data = [family, n, p, intercept, flags, s_1..s_Dc, (m_tau, s_tau: families 2, 3), y_1..y_n,
                              o_1..o_n (flags & 1), w_1..w_n (flags & 2), X (n x p, row-major)], flags in {1, 2, 3} (0 is
                              SMCN_MODEL_GLM's model: refused).  o finite; w finite and >= 0, at least one > 0.  A row with
                              w_i = 0 adds exactly 0 to llik and to every gradient sum whatever its term is (an overflowing
                              e^eta_i included), and the families' -inf rules look at the rows with w_i != 0 only.
                              Pointwise log-likelihoods, prediction and predictive draws as for SMCN_MODEL_GLM (new rows:
                              [family, m, p, intercept, flags, y, o (flags & 1), w = 1.. (flags & 2), X]); the pointwise
                              criteria and PSIS-LOO are refused for a fit with weights (flags & 2) */
/* (11 is unassigned: refused as an unknown model id) */
#define SMCN_MODEL_CGLM 12   /* continuous-response GLM, SMCN_MODEL_GLM's linear predictor and coefficient priors with a scale
                              coordinate: data = [family (0 gamma_log, 1 student_t), n, p, intercept, df (0 for gamma_log),
                              s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, row-major)], Dc = p + intercept >= 1,
                              x = (b_1..b_Dc, tau), D = Dc + 1 <= 64, b_c ~ N(0, s_c^2), tau ~ N(m_tau, s_tau^2);
                                family 0: y_i ~ Gamma(shape a = e^tau, rate a / e^eta_i) (mean e^eta_i), y finite and > 0;
                                family 1: y_i ~ student_t(df, eta_i, sigma = e^tau), df finite and > 0 fixed by the caller,
                                          y finite;
                              constrain reports (b, e^tau).  llik = -inf where e^tau (gamma) or e^-tau (student_t) leaves
                              the normal range, where e^-eta_i overflows (gamma) and where (y_i - eta_i) e^-tau overflows
                              (student_t).  The pointwise criteria, PSIS-LOO, calibration, prediction and predictive draws
                              are refused for this model */

#define SMCN_LKERNEL_FORWARD 0  /* smcnuts/lkernel/forward_lkernel.py:22-35   */
#define SMCN_LKERNEL_GAUSSIAN 1 /* smcnuts/lkernel/gaussian_lkernel.py:24-84  */

/* per-particle flag bits returned by smcn_get_tree_stats */
#define SMCN_FLAG_TAPE_OVERFLOW 1

int smcn_version(void);
const char* smcn_last_error(const smcn_ctx* ctx);

/* One context per GPU: replaces the state held by Samples.__init__ /
 * initialise_samples (smcnuts/samples/samples.py:8-88) and the target object.
 * `particle_base` is the global index of this shard's first particle (Philox
 * streams are keyed by global particle index, so a sharded run draws the same
 * numbers as a single-GPU run). */
int smcn_ctx_create(smcn_ctx** out, int device_id, int64_t n_particles, int64_t particle_base,
                    int model_id, const double* model_data, int64_t model_data_len);
void smcn_ctx_destroy(smcn_ctx* ctx);
int smcn_dim(const smcn_ctx* ctx);
int smcn_constrained_dim(const smcn_ctx* ctx);
/* 1 if this context's NUTS kernel can run several SMC iterations per launch (smcn_fuse_* /
 * smcn_block_* with B > 1), 0 if it runs one NUTSProposal.rvs (proposal/nuts.py:34-56) per launch. */
int smcn_fused_transitions(const smcn_ctx* ctx);
/* Use a caller-provided hipStream_t (e.g. the framework's current stream). */
int smcn_set_stream(smcn_ctx* ctx, void* hip_stream);
int smcn_synchronize(smcn_ctx* ctx);

/* Philox4x32-10 seed of the production RNG (replaces the shared sequential
 * np.random stream). */
int smcn_set_seed(smcn_ctx* ctx, uint64_t seed);

/* Particle state in/out (Samples.x / logw / r / x_new / r_new). NULL = skip. */
int smcn_set_state(smcn_ctx* ctx, const double* x, const double* logw);
int smcn_get_state(smcn_ctx* ctx, double* x, double* logw, double* wn);
int smcn_get_proposal(smcn_ctx* ctx, double* r, double* x_new, double* r_new, double* logw_new);
int smcn_set_momentum(smcn_ctx* ctx, const double* r);
/* A proposal computed elsewhere -- forward_kernel.rvs(x, r, phi) -> (x', r'), samples/samples.py:158 -- e.g. the
 * reference's recorded one: uploads r, x', r' and evaluates the density parts at x and x', leaving the state
 * smcn_propose_nuts leaves (the re-weight, L-kernels and tempering then run on it unchanged). */
int smcn_set_proposal(smcn_ctx* ctx, const double* r, const double* x_new, const double* r_new);

/* StanModel.logpdf / logpdfgrad / constrain (model/bridgestan.py:28-120) on
 * M rows of x; lpri/llik are the prior(+Jacobian) and likelihood parts with
 * log pi_phi = lpri + phi * llik.  Any output may be NULL. */
int smcn_target_eval(smcn_ctx* ctx, const double* x, int64_t M, double phi, double* logp,
                     double* grad, double* lpri, double* llik);
int smcn_target_constrain(smcn_ctx* ctx, const double* x, int64_t M, double* out);

/* Initial particles: x ~ N(0, I) from Philox stream 3 and
 * logw = log pi_phi(x) - N(x; 0, I)  (samples.py:77,85 with the harness'
 * sample_proposal, experiments/run_experiments.py:110). */
int smcn_init_particles_std_normal(smcn_ctx* ctx, double phi);
/* logw = log pi_phi(x) - logq0 for caller-supplied x (set_state) and q0. */
int smcn_init_weights(smcn_ctx* ctx, double phi, const double* logq0);

/* Samples.normalise_weights + calculate_ess (samples.py:91-113), split so
 * that shards can be combined: partials = [max, count_of_max, sum exp(.-max)
 * over non-max, sum exp(2(.-max)) over all finite-or-+inf].  apply() takes the
 * GLOBAL log-likelihood and writes wn = exp(logw - loglik). */
int smcn_normalise_partials(smcn_ctx* ctx, double out[4]);
int smcn_normalise_apply(smcn_ctx* ctx, double loglik);
/* Single-shard convenience: both steps; returns loglik and ESS. */
int smcn_normalise(smcn_ctx* ctx, double* loglik, double* ess);

/* Estimate.return_estimate (estimate/estimate.py:38-57,79-95) in constrained
 * space, two passes as the reference: sums[Dc] = sum_i wn_i * c(x_i), then
 * sums[Dc] = sum_i wn_i * (c(x_i) - mean)^2. */
int smcn_moment_sums(smcn_ctx* ctx, const double* mean_or_null, double* sums);

/* Samples._resample (samples.py:124-146): multinomial through
 * cdf = cumsum(wn)/sum, idx = searchsorted(cdf, u, 'right'), x <- x[idx],
 * logw <- loglik - log(n_total).  u = NULL draws Philox stream 2.
 * idx_out (int64[N], may be NULL) receives the ancestor indices. */
int smcn_resample_multinomial(smcn_ctx* ctx, const double* u, double loglik, double log_n_total,
                              int64_t iteration, int64_t* idx_out);
/* Resampling scheme for every resampling entry point of the ctx.  SMCN_RESAMPLE_MULTINOMIAL (default)
 * is the reference's rng.choice (samples.py:139): N independent uniforms, searchsorted right.
 * SMCN_RESAMPLE_SYSTEMATIC draws ONE uniform u0 per resampling and uses the keys (i + u0) / N on the
 * same prefix sum and search (lower-variance alternative; not in the reference). */
#define SMCN_RESAMPLE_MULTINOMIAL 0
#define SMCN_RESAMPLE_SYSTEMATIC 1
int smcn_set_resample_scheme(smcn_ctx* ctx, int scheme);
/* NUTSProposal.rvs (nuts.py:34-56) in the lane-per-particle kernel (arma): a launch lasts as long as its longest chain
 * of leaves, so when at most 16 (8, 4, 2, 1) lanes of a wavefront are still building trees, 4 (8, 16, 32, 64) lanes
 * share each one's T-step recurrence (segmented scan, csrc/smcn_nuts3.hpp recur_wide).  The sums are then re-associated: results agree
 * with the one-lane evaluation to rounding (~1e-15 relative on the density), not bit for bit, and WHICH evaluations
 * run wide depends on the launch's schedule (iterations per launch, wave mates).  1 (default) = on; 0 = every
 * evaluation by one lane (bit-identical results whatever the schedule: what the fused-vs-stepwise tests pin). */
int smcn_set_wide_eval(smcn_ctx* ctx, int on);
/* The lane kernel's tree bookkeeping.  A tree takes an even number of loop iterations unless a leaf diverges, so in every
 * other iteration all leaves of a wavefront are even ones: they park at level 0 and nothing else happens.  1 (default):
 * such an iteration, found by one ballot, passes over the merge, top-level and tree-end code in one branch, and an
 * iteration in which no lane starts a tree or a doubling over the start code; 0: every iteration takes the generic code.
 * The results are the same bits either way: the schedule, the draws and the arithmetic do not change. */
int smcn_set_phase_paths(smcn_ctx* ctx, int on);
/* The lane kernel with a lane per particle: when a lane's trees start.  A tree takes 2^depth loop iterations, so the lanes of
 * a wavefront, which all start in iteration 0, reach the leaves with many merges in the same iterations -- until one tree
 * stops early (a sub-tree U-turn, a depth-1 tree, a divergent leaf) and its lane is out of step for the rest of the
 * launch.  n = 1, 2, 4 (default) or 8: a lane whose tree ended starts the next one in the first iteration whose number is
 * a multiple of n, sitting out up to n - 1 iterations; 1 = in the very next iteration.  Only when a tree runs changes:
 * with smcn_set_wide_eval(0) the results are the same bits for every n.  (Fewer lanes than particles, smcn_set_lane_grid:
 * the lane queue has its own rule of this kind and ignores this setting.) */
int smcn_set_tree_align(smcn_ctx* ctx, int n);
/* Loop iterations each wavefront of the last lane-kernel launch ran, the first n wavefronts' (n at most the launch's number
 * of wavefronts: a wavefront per 64 particles unless smcn_set_lane_grid caps them).  A lane per particle: the largest, over
 * the wavefront's lanes, of the iteration its last tree ended in, plus one -- what smcn_set_tree_align changes. */
int smcn_get_wave_iterations(smcn_ctx* ctx, uint32_t* out, int64_t n);
/* The lane kernel's schedule: at most `waves` wavefronts are launched (0 = default: one per SIMD, all the chip holds of this
 * kernel; < 0: no cap, one per 64 particles).  With fewer lanes than particles every wavefront owns a contiguous run of
 * particles (N / waves of them) and its 64 lanes work through it, so a population that is no multiple of 65 536 per GPU
 * does not pay a second round of wavefronts.  Which lane runs a particle never changes its draws (Philox is keyed by the
 * particle); with smcn_set_wide_eval(0) the results are bit-identical under every schedule.  (More than 4 096 particles
 * per wavefront: the launch falls back to one wavefront per 64 particles.) */
int smcn_set_lane_grid(smcn_ctx* ctx, int64_t waves);
/* ... and then a particle's block of B fused transitions is worked off in `segments` pieces (0 = auto: 4; 1 = a lane keeps
 * its particle for the whole block): a lane that starts the last transition of its segment looks for a ready job of its
 * wavefront -- another particle's next segment, the least advanced first --; if there is one it leaves its own particle's
 * (x', running log-weight) in a hand-over record at the segment's end and goes over to that job without an idle
 * iteration, else it simply goes on with its own particle.  The work is the same trees in the same order per particle;
 * only who builds them changes (bit-identical results with smcn_set_wide_eval(0)). */
int smcn_set_lane_segments(smcn_ctx* ctx, int segments);

/* Two-phase NUTS launches (the group kernel whose trajectory edges live in registers: PRMwCD).
 * A launch of the group kernels lasts as long as its longest tree; with doublings > 0 a tree that still wants a doubling
 * after that many is parked at the boundary (its state: the two edges, the selected sample, a few scalars) and finished by
 * a second launch behind the first.  widen != 0: by the wavefront-per-particle functor of the model where one exists
 * (PRMwCD: 100 observations over 64 lanes; results then differ from the one-launch run by the rounding of the
 * re-associated likelihood sums), else by the kernel that parked it (bit for bit the one-launch result).
 * widen == 2 (tests, A/B): nothing is parked -- every tree runs from its start in the kernel that otherwise finishes the
 * parked ones, so that the parity tests reach the finisher's functor and tree stack on whole trees.
 * doublings <= 0: one launch (the default).  smcn_nuts_parked: how many trees the last proposal parked. */
int smcn_set_nuts_cap(smcn_ctx* ctx, int doublings, int widen);
int smcn_nuts_parked(smcn_ctx* ctx, int64_t* parked);
/* An INNER park level of the first launch (PRMwCD's lane-group kernel; 0 < doublings < the cap above, 0 = none): a tree
 * that wants more than `doublings` doublings is parked there as well and taken up again BY THE SAME LAUNCH once every fresh
 * particle has been handed out, so that the launch ends on pieces of trees (at most 2^(cap-1) leaves) instead of on whole
 * ones.  The same trees in another order: results are bit-identical with and without it. */
int smcn_set_nuts_requeue(smcn_ctx* ctx, int doublings);

/* Samples.propose_samples (samples.py:149-158) = momentum draw +
 * NUTSProposal.rvs (proposal/nuts.py:34-175) for every particle in ONE launch.
 * Momentum: Philox stream 1 unless smcn_set_momentum was called since the
 * last proposal.  Tape mode (tests): tape/tape_off as recorded from the
 * reference, tape_off has N+1 entries; NULL = Philox stream 0. */
int smcn_propose_nuts(smcn_ctx* ctx, double step_size, double phi, int max_depth, double delta_max,
                      int64_t iteration, const double* tape, const int64_t* tape_off);
/* per-particle leapfrog count, doublings, draws consumed, flags (int32[N]). */
int smcn_get_tree_stats(smcn_ctx* ctx, int32_t* nleap, int32_t* depth, int32_t* ndraws, int32_t* flags);
/* sum of leapfrogs of the last proposal (device-side reduction). */
int smcn_last_leapfrogs(smcn_ctx* ctx, int64_t* total);
/* density parts at x (before) and x_new (after) kept by the last proposal. */
int smcn_get_density_parts(smcn_ctx* ctx, double* lpri0, double* llik0, double* lpri1, double* llik1);

/* Samples._non_asympototic_reweight (samples.py:183-196):
 * logw_new = logw + pi_1(x_new) - pi_1(x) + L - q with the N(0,I) momentum
 * proposal.  FORWARD: L = N(-r_new; 0, I).  GAUSSIAN: L supplied per particle
 * through smcn_gauss_lkernel_logpdf beforehand. */
int smcn_reweight(smcn_ctx* ctx, int lkernel);
/* The asymptotic strategy (lkernel "asymptoticLKernel"):
 *  - smcn_accept_reject: the Metropolis step of NUTSProposalWithAccRej.rvs
 *    (smcnuts/proposal/nuts_acc_rej.py:42-49, proposal/utils.py:3-34) on the last
 *    proposal; u = NULL draws Philox stream 4; a rejected particle keeps (x, r);
 *  - smcn_reweight_asymptotic: Samples._asymptotic_reweight (samples.py:169-180),
 *    logw_new = logw + pi_{phi_new}(x) - pi_{phi_old}(x) at the OLD positions;
 *  - smcn_set_logw_density_ratio: logw = pi_{phi_num}(x) - pi_{phi_den}(x) at the resident
 *    x (estimate/estimate_from_tempered.py:47). */
int smcn_accept_reject(smcn_ctx* ctx, double phi, const double* u, int64_t iteration);
int smcn_reweight_asymptotic(smcn_ctx* ctx, double phi_old, double phi_new);
int smcn_set_logw_density_ratio(smcn_ctx* ctx, double phi_num, double phi_den);

/* Plug-in values for a duck-typed momentum proposal (lkernel.calculate_L /
 * forward_kernel.logpdf evaluated by the caller): per-particle L and/or q used
 * by the next smcn_reweight instead of the N(0, I) closed forms. */
int smcn_set_lkernel_values(smcn_ctx* ctx, const double* L, const double* q);

/* GaussianApproxLKernel.calculate_L (gaussian_lkernel.py:45-82), N-scaled
 * parts: sums[2D + 2D*2D] = [sum X, sum X X^T] of X = [-r_new, x_new] shifted
 * by `shift[2D]` (pass the previous mean, or zeros); then given the D x D
 * regression matrix B, offset m0[D], whitening U[D,D] and constant c0 the
 * per-particle log-density L_i = c0 - 0.5 |U^T(-r_i - m0 - B (x_i - mu_x))|^2. */
int smcn_gauss_lkernel_sums(smcn_ctx* ctx, const double* shift, double* sums);
int smcn_gauss_lkernel_logpdf(smcn_ctx* ctx, const double* mu_x, const double* m0, const double* B,
                              const double* U, double c0);
/* The same L-kernel for ONE shard with the D x D algebra on the device (two Cholesky factorisations by one wavefront; D <= 32):
 * both moment passes, the algebra and the conditional log-density are enqueued back to back, one wait at the end.
 * info = [status, c0, cond(c_xx), cond(cov)] (condition numbers: upper estimates).  status 0: the L values are set as
 * by smcn_gauss_lkernel_logpdf.  status 1 / 2: a covariance is not positive definite / too ill-conditioned for that route
 * (estimate >= 1e8) -- nothing is set, and the caller runs the reference's own pinv / eigh with their cut-offs and
 * exceptions through smcn_gauss_lkernel_sums + smcn_gauss_lkernel_logpdf (gaussian_lkernel.py:45-82). */
int smcn_gauss_lkernel_device(smcn_ctx* ctx, double info[4]);
/* The same over SEVERAL shards ("Gaussian L-kernel -- all-gather of 2D + (2D)^2 sums"): every rank runs
 *   stage 0 (this shard's un-shifted sums)  -> all-gather of nq = 2D + 2D (2D + 1) / 2 doubles, local -> gathered
 *   stage 1 (rows added in rank order, mean over n_total, this shard's centred sums)  -> the same all-gather
 *   stage 2 (rows added, the D x D algebra -- the same bits on every rank --, the log-density of this shard's particles;
 *            waits; info as above, status 1 / 2 handled as above)
 * on the two device buffers smcn_gauss_lkernel_buffers names (gathered = [world][nq], rank order).  world == 1: no
 * exchange, the stages read the local row.  On status 1 / 2 the L values the caller had set are left untouched. */
int smcn_gauss_lkernel_buffers(smcn_ctx* ctx, int world, void** local_dev, void** gathered_dev);
int smcn_gauss_lkernel_stage(smcn_ctx* ctx, int stage, int world, double n_total, double info[4] /* stage 2 */);

/* ESSTempering._ess (tempering/adaptive_tempering.py:41-56) partials at
 * new_phi for logw = new_phi*loglik + logpri - base, with base = pi_{phi_old}
 * at x_new; same 4 partials as smcn_normalise_partials. */
int smcn_temper_partials(smcn_ctx* ctx, double phi_old, double phi_new, double out[4]);
/* ESSTempering.calculate_phi (adaptive_tempering.py:18-63) with the bisection's own iteration on the device
 * (csrc/smcn_temper.hpp: scipy/optimize/Zeros/bisect.c restated; a pass evaluates the 15 trial points of the next four
 * bisection steps, a one-wavefront kernel takes the steps).  target = alpha N (the ESS the weights are tempered to);
 * the density parts at x_new must be resident (kept by the NUTS kernel / smcn_eval_proposed_parts).
 *   one shard:      smcn_temper_bisect -- one host synchronisation when ESS(1) >= target (phi stays 1), two when a
 *                   bisection runs, instead of one per trial point;
 *   several shards: per pass  smcn_temper_bisect_pass; all-gather of the [15][4] doubles of smcn_temper_bisect_buffers
 *                   (in the stream); smcn_temper_bisect_decide -- all asynchronous -- and smcn_temper_bisect_result
 *                   after pass 10 (status 1: enqueue further passes, up to 25).
 * status: 0 = *phi holds the result (1.0 if ESS(1) >= target); 2 = f(phi_old), f(1) of equal sign (scipy: ValueError);
 * 3 = no convergence in 100 steps (scipy: RuntimeError). */
int smcn_temper_bisect(smcn_ctx* ctx, double phi_old, double target, double* phi, int* status);
int smcn_temper_bisect_pass(smcn_ctx* ctx, int pass, double phi_old);
int smcn_temper_bisect_buffers(smcn_ctx* ctx, int world, void** local, void** gathered);
int smcn_temper_bisect_decide(smcn_ctx* ctx, int pass, int world, double target, double phi_old);
int smcn_temper_bisect_result(smcn_ctx* ctx, double* phi, int* status);

/* Density parts (lpri, llik) at the resident x (which = 0) or x_new (1), for
 * the first temperature of Samples.initialise_samples (samples.py:78-82). */
int smcn_eval_proposed_parts(smcn_ctx* ctx, int which);

/* Samples.update_samples (samples.py:215-222) + the acceptance statistic of
 * SMCSampler.update_sampler (smc_sampler.py:97): x <- x_new, logw <- logw_new;
 * n_moved = #particles with every coordinate changed. */
int smcn_commit(smcn_ctx* ctx, int64_t* n_moved);

/* ---- device-resident loop (forward L-kernel, fixed temperature) -------------
 * The order of SMCSampler.sample() (smc_sampler.py:109-149) with every scalar
 * (log-likelihood, ESS, the resample decision of samples.py:120, estimates,
 * leapfrog and acceptance counts) produced and consumed on the device: K
 * iterations are enqueued without a host round trip.
 *   smcn_fast_begin   allocates the per-iteration history (K+1 records of
 *                     6 + 2*Dc doubles: ll, ess, resampled, leapfrogs, moved,
 *                     phi, mean[Dc], var[Dc]) and, if save_history, x_saved /
 *                     logw_saved (smc_sampler.py:73-74) on the device.
 *   smcn_step_begin   shard partials [max, count, s1, s2, sum w c(x), sum w
 *                     (c(x)-shift)^2] of the current weights into the buffer
 *                     smcn_fast_buffers reports (4 + 2*Dc doubles).
 *   (several shards: all-gather `local_partials` of every rank into `gathered`,
 *    rank-major, on the same stream -- the ONLY exchange of an iteration)
 *   smcn_step_finish  combines the shards in rank order, then normalise,
 *                     estimate, ESS, conditional multinomial resampling (local
 *                     to the shard), momentum draw, NUTS, re-weight, commit,
 *                     history.  last != 0: only the closing normalise /
 *                     estimate / ESS of smc_sampler.py:143-149.
 *   smcn_fast_read    synchronises and downloads. */
int smcn_fast_begin(smcn_ctx* ctx, int64_t K, int save_history, int world);
int smcn_fast_buffers(smcn_ctx* ctx, void** local_partials, void** gathered, int* nq);
int smcn_set_resample_uniforms(smcn_ctx* ctx, const double* u);
int smcn_step_begin(smcn_ctx* ctx, int64_t k);
int smcn_step_finish(smcn_ctx* ctx, int64_t k, int world, int rank, double n_total, double step_size,
                     double phi, int max_depth, double delta_max, int lkernel, int last,
                     const double* tape, const int64_t* tape_off);
int smcn_fast_read(smcn_ctx* ctx, double* hist, double* x_saved, double* logw_saved);
/* The same for generations k_from .. K only, and -- beside the loop -- generations k_from .. k_to that the caller knows to be
 * final (their blocks have been waited for), on a stream of the library's own: the copies then run under the NUTS launch
 * that is already enqueued instead of behind the whole run (SMCSampler.sample(): smc_sampler.py:139-140 keeps x_saved /
 * logw_saved of every generation). */
int smcn_fast_read_from(smcn_ctx* ctx, double* hist, double* x_saved, double* logw_saved, int64_t k_from);
int smcn_history_download(smcn_ctx* ctx, int64_t k_from, int64_t k_to, double* x_saved, double* logw_saved);
/* ---- fused transitions: B SMC iterations per NUTS launch ---------------------
 * Between two resampling events a particle's next NUTS transition depends only
 * on its own sample, so B iterations of the loop (smc_sampler.py:109-140) can
 * run inside one launch, speculating that no generation in between falls below
 * the resampling threshold (samples.py:120); the speculation is checked on the
 * recorded weights and rolled back to the first generation that has to
 * resample, so results equal the one-iteration-per-launch schedule bit for bit.
 *   smcn_fuse_begin(Bmax, world)   after smcn_fast_begin
 *   per block of B <= Bmax iterations starting at k0:
 *     smcn_step_begin(k0); [exchange local_partials -> gathered]
 *     smcn_fuse_run(k0, B, ...);   [exchange the (B-1) x nq block of smcn_fuse_buffers]
 *     smcn_fuse_finish(k0, B, ..., &n_ok)    n_ok in 1..B iterations were valid;
 *                                            the resident state is generation k0 + n_ok. */
int smcn_fuse_begin(smcn_ctx* ctx, int Bmax, int world);
int smcn_fuse_buffers(smcn_ctx* ctx, void** local_partials, void** gathered, int* nq);
int smcn_fuse_run(smcn_ctx* ctx, int64_t k0, int B, int world, int rank, double n_total, double step_size,
                  double phi, int max_depth, double delta_max, int decided);
/* decided = 0: resampling decision + shard-local multinomial resampling on the device (one shard:
 * the reference's; several shards: each keeps its own mass, logw = log W_shard - log N_local).
 * Several shards, default: resampling is GLOBAL (Samples._resample, samples.py:124-146, over the whole
 * population -- the indices one shard of N_total particles would draw), so results do not depend on
 * the shard count (to rounding; BIT FOR BIT only with smcn_set_wide_eval(0): the default lets lane groups evaluate a
 * wavefront's stragglers, and which evaluations those are depends on the schedule, hence on the shard sizes).  Per block: smcn_step_begin(k0); exchange; smcn_fuse_decide(k0, .., &resample);
 * if resample: the routed global resampling (smcn_gres_*: tile totals, then keys and ancestor rows point to
 * point -- the population itself is never gathered); finally smcn_fuse_run(.., decided = 1). */
int smcn_fuse_decide(smcn_ctx* ctx, int64_t k0, int world, int rank, double n_total, double phi, int* resample);

/* Pipelined form of the fused block (same arithmetic as smcn_fuse_run/_finish; smc_sampler.py:109-140
 * for B iterations).  The statistics of ALL B generations are produced at the end of the block (one
 * combine launch; history rows come back through pinned memory behind an event), so the caller can
 * enqueue the next block -- speculating "no resampling" -- BEFORE waiting, and the device never idles
 * on the host.  Per block:
 *   [smcn_step_begin + exchange + smcn_fuse_decide (+ smcn_block_resample_local | global resampling)]
 *   smcn_block_launch(k0, B)          momentum draws, B NUTS transitions per particle
 *   smcn_block_post(k0, B, world)     generations k0+1..k0+B, re-weight, counts, shard partials [B][nq]
 *   exchange of smcn_fuse_buffers     (in stream: RCCL on the device pointers; or smcn_block_partials_get/_set)
 *   smcn_block_stats(k0, B, ..)       history rows k0+1..k0+B; read-back enqueued
 *   smcn_block_commit(k0, B) + smcn_block_launch(k0+B, B')      optional: the speculative next block
 *   smcn_block_wait(B, &n_ok, &resample_next)
 * If n_ok < B or resample_next: discard the speculative launch (smcn_synchronize), smcn_block_commit(k0,
 * n_ok) and restart from generation k0 + n_ok, which resamples. */
/* Targets evaluated by the CALLER: any model with the reference's StanModel interface
 * (smcnuts/model/bridgestan.py:28-120: log_density / log_density_gradient of an arbitrary BridgeStan
 * model) that has no device functor.  A context created with SMCN_MODEL_HOST asks this function for
 * the density wherever the device functors would be evaluated: x is [n][D] row-major; lpri/llik [n]
 * receive log prior (+ Jacobian) and log likelihood, so that log pi_phi = lpri + phi * llik; with
 * want_grad != 0 also gpri/glik [n][D].  Non-finite values are mapped to -inf as bridgestan.py:45-49
 * does.  Return 0, or non-zero to abort the calling entry point.  The NUTS proposal then runs the
 * tree building on the device and the target in lock step on the host (one call per leapfrog of the
 * longest tree): the generality path, not the fast one.  Device-resident loops (smcn_fast_*,
 * smcn_block_*) are not available for such a context. */
typedef int (*smcn_host_target_fn)(void* user, int64_t n, int D, const double* x, int want_grad, double* lpri,
                                   double* llik, double* gpri, double* glik);
int smcn_set_host_target(smcn_ctx* ctx, smcn_host_target_fn fn, void* user);
/* sum_i wn_i v_ic  or  sum_i wn_i (v_ic - shift_c)^2 over caller-supplied rows v [N][Dc] (estimate.py:79-95
 * with the caller's own constrain(), bridgestan.py:100-120); out has Dc entries. */
int smcn_moment_sums_of(smcn_ctx* ctx, const double* v, int Dc, const double* shift, double* out);

int smcn_block_resample_local(smcn_ctx* ctx, int64_t k0);
int smcn_block_launch(smcn_ctx* ctx, int64_t k0, int B, double step_size, double phi, int max_depth,
                      double delta_max);
int smcn_block_post(smcn_ctx* ctx, int64_t k0, int B, int world);
int smcn_block_partials_get(smcn_ctx* ctx, int B, double* out);
int smcn_block_partials_set(smcn_ctx* ctx, int B, int world, const double* gathered);
int smcn_block_stats(smcn_ctx* ctx, int64_t k0, int B, int world, int rank, double n_total, double phi,
                     int final_block /* the run ends with this block: the scalar history is downloaded behind it */);
int smcn_block_wait(smcn_ctx* ctx, int B, int* n_ok, int* resample_next);
int smcn_block_commit(smcn_ctx* ctx, int64_t k0, int n_ok);
/* What smcn_block_post / smcn_block_stats enqueue behind the NUTS launch of an arma block.  1 (default): one streaming
 * kernel (unpack + re-weight + the generations + their block partials, from registers) and one tail kernel (shard
 * partials, counts and, one shard, the combine of smcn_block_stats, which then launches nothing when it brings the
 * launch's phi and n_total = N).  0: the separate launches these replace (post, counts, partials, reduce, copy, combine
 * behind counters cleared in front of the NUTS launch).  Every output has the same bits either way; 0 is the reference of
 * tests/test_gpu_block_post.py.  Blocks of 4 and more transitions over more than 131 072 particles a shard run the
 * separate launches under both. */
int smcn_set_block_post(smcn_ctx* ctx, int mode);
/* ESS (samples.py:113) of the B generations of the block smcn_block_wait returned for. */
int smcn_block_ess(smcn_ctx* ctx, int B, double* out);
int smcn_fuse_finish(smcn_ctx* ctx, int64_t k0, int B, int world, int rank, double n_total, double phi,
                     int* n_ok);
#ifdef SMCN_LEGACY_ABI   /* round-1 generation of the block exchange: nothing in this repository calls it any more
                          * (smcn_block_partials_get / _set replaced it); exported only by builds that define the macro */
int smcn_fuse_partials_get(smcn_ctx* ctx, int B, double* out);
int smcn_fuse_partials_set(smcn_ctx* ctx, int B, int world, const double* in);
#endif

/* Host-side exchange of the shard partials, for communicators that cannot
 * all-gather device memory (e.g. gloo): read this shard's 4 + 2*Dc doubles /
 * write the world x (4 + 2*Dc) gathered block. */
int smcn_partials_get(smcn_ctx* ctx, double* out);
int smcn_partials_set_gathered(smcn_ctx* ctx, const double* in, int world);

/* NUTS kernel time measured with HIP events on the launch stream since the
 * last reset: out = [total ms, launches, 0, 0, 0, 0]; reset != 0 clears. */
int smcn_timers(smcn_ctx* ctx, double out[6], int reset);

/* Self test of the library's lean fp64 device math used inside the arma density and of its wavefront reduction:
 * out[0..n) = exp(x), out[n..2n) = log1p(|x|), out[2n..3n) = 1/x, out[3n..4n) = the sum of x over the element's
 * wavefront (64 consecutive elements; the butterfly of the NUTS kernels, last stages by v_permlane*_swap),
 * out[4n..5n) = the same butterfly through ds_bpermute (identical bits expected); out[5n..7n) = the wavefront sums of
 * x and x^2 by the fused two-value butterfly (wave_sum2), out[7n..11n) = those of x, x^2, |x|, 1 - x by the four-value
 * one (wave_sum4).  out holds 11 n doubles. */
int smcn_selftest_math(smcn_ctx* ctx, const double* x, int64_t n, double* out);
/* Measurement aid (bench.py, roofline.peak_measured; SURVEY.md 8(d) asks for nominal AND on-box denominators): the
 * device's streaming copy rate [GB/s] and its fp64 FMA rate [TFLOP/s] at one and at four wavefronts per SIMD. */
int smcn_measure_peaks(smcn_ctx* ctx, double out[3]);
/* Device memory the library holds beyond its contexts: a context's streams and buffers are not given back to the driver
 * when it is destroyed (creating a stream costs 2-9 ms; fresh buffers cost their first touch); they are pooled per device
 * and handed to the next context
 * (buffers: to a request of the same size, zeroed).  The cache holds at most `SMCN_DEVICE_CACHE_MB` megabytes per device
 * (environment, read once; default 3072; 0 = every buffer goes back to the driver at once) and is emptied when an
 * allocation fails.  smcn_device_cache_trim returns what is idle on `device` (-1: all devices) to the driver and
 * reports the bytes released; *idle_bytes (may be NULL) = what was idle before. */
int smcn_device_cache_trim(int device, int64_t* released_bytes, int64_t* idle_bytes);
/* Test hook for smcn_set_wide_eval: the four sums of the arma recurrence (sum err^2 and its three sensitivity sums) of
 * n rows x[n][4], by one lane (out[i][0..3]) and by a group of `lanes` (64, 32, 16, 8 or 4) lanes (out[i][4..7]). */
int smcn_selftest_wide(smcn_ctx* ctx, int lanes, const double* x, int64_t n, double* out);
/* Test hook for the settled mu-sensitivity of the arma recurrence: n rows x[n][4], 64 consecutive rows
 * to a wavefront in row order.  out[i][0..3] = the four sums of the full recurrence, out[i][4..7] = those of the form the
 * kernels run (the mu-sensitivity no longer updated once it repeats with period <= 2 on every lane of the wavefront),
 * out[i][8] = the number of full steps before that wavefront switched (0: it never did).  Arma contexts only. */
int smcn_selftest_recur(smcn_ctx* ctx, const double* x, int64_t n, double* out);

/* ---- shards: one process per GPU; the reference has no counterpart (single thread) ----
 * In-library communicator: RCCL over xGMI (looked up at run time; no link-time dependency).  Rank 0 obtains the
 * 128-byte id and hands it to the other ranks by any means (smcnuts_amd.parallel.RcclComm: a file keyed by the
 * launch, one node); collectives run in the context's stream on device pointers. */
int smcn_comm_unique_id(char out[128]);
int smcn_comm_init(smcn_ctx* ctx, int rank, int world, const char id[128]);
int smcn_comm_destroy(smcn_ctx* ctx);
/* The communicator's own view: out = [ranks in it (ncclCommCount), this rank (ncclCommUserRank), RCCL version code];
 * -1 each when the context has no communicator.  bench.py prints it so that a multi-GPU line proves how many ranks RCCL saw. */
int smcn_comm_info(smcn_ctx* ctx, int out[3]);
int smcn_comm_allgather(smcn_ctx* ctx, const void* src_dev, void* dst_dev, int64_t n_doubles);
int smcn_comm_allgather_host(smcn_ctx* ctx, const double* src, int64_t n_doubles, double* dst /* [world][n] */);
int smcn_comm_alltoallv(smcn_ctx* ctx, const void* send_dev, const int64_t* send_counts, void* recv_dev,
                        const int64_t* recv_counts, int elem_doubles);
int smcn_buf_get(smcn_ctx* ctx, const void* dev, int64_t n_doubles, double* host);
int smcn_buf_set(smcn_ctx* ctx, void* dev, int64_t n_doubles, const double* host);
/* device -> device in the context's stream, NOT waited for: several shards of one process on one GPU exchange their
 * buffers with it (smcnuts_amd.parallel.InProcessComm -- the rehearsal of the shard protocol a one-GPU box allows). */
int smcn_buf_copy(smcn_ctx* ctx, void* dst_dev, const void* src_dev, int64_t n_doubles);

/* Samples._resample (samples/samples.py:124-146: rng.choice over the WHOLE population) across shards without
 * gathering the population: blocked scan per shard -> all-gather of the tile totals (N_local / 1024 doubles) ->
 * every rank plans its keys (Philox by global slot) and their owner ranks -> all-to-all of the keys -> the owners
 * search their tiles and gather the ancestor rows -> all-to-all of only those rows -> scatter.  The ancestors are
 * those one shard of N_total particles draws.  Shards of ANY size: where N_local is a multiple of the scan tile (1024) the
 * cdf is summed exactly as one shard of N_total sums it; otherwise the last tile of every shard is partial and an
 * ancestor can differ from the one-shard run only at keys within rounding of a cdf step. */
int smcn_gres_begin(smcn_ctx* ctx, int world, double* ttot_host /* [N_local/1024] or NULL */);
int smcn_gres_buffers(smcn_ctx* ctx, void** ttot_local, void** ttot_all, void** keys_send, void** keys_recv,
                      void** rows_send, void** rows_recv);
int smcn_gres_plan(smcn_ctx* ctx, int world, int rank, const double* ttot_all_host /* or NULL: already on the device */,
                   int64_t iteration, int32_t* dest_rank_host /* [N_local] */);
int smcn_gres_set_order(smcn_ctx* ctx, const int32_t* order /* [N_local]: slot of the k-th key in send order */);
int smcn_gres_reserve(smcn_ctx* ctx, int64_t n_requests_to_serve);
int smcn_gres_serve(smcn_ctx* ctx, int world, int rank, int64_t n_requests);
int smcn_gres_finish(smcn_ctx* ctx, int world, const double* loglik /* NULL: the device-resident loop's */);

/* Measurement aid: `reps` x the kernels of Samples._resample (samples/samples.py:124-146) on the resident
 * state, timed with HIP events on the context's stream (bench.py's roofline entry for resampling). */
int smcn_bench_resample(smcn_ctx* ctx, int reps, int64_t iteration, double* ms_total);

/* ---- pointwise log-likelihood and predictive criteria (SMCN_MODEL_GLM, all four families, D <= 64, any n) ----
 * ll[p][i] = log p(y_i | x_p), the per-observation term exactly as the density forms it (sum_i ll[p][i] is the llik of
 * smcn_target_eval; the -lgamma(y + 1) constants included), finite or -inf.  Contexts of every other model fail with a
 * message (smcn_last_error) that says so.  SMCN_MODEL_OGLM with offsets alone (flags = 1) is served as SMCN_MODEL_GLM,
 * eta_i taking o_i; with weights (flags & 2) these functions and smcn_psis_* fail with a message of their own: the
 * criteria of a weighted fit are not implemented.
 *
 * smcn_pointwise_dims: n and the column count Q (= 11) of a partials block.
 * smcn_pointwise_loglik: ll as [M][n] row-major for M caller-supplied points x[M][D] (the plain form, for problems small
 * enough to hold the matrix).
 * smcn_pointwise_partials: the weighted reductions OVER PARTICLES per observation, without the matrix, as MERGEABLE
 * partials out[1 + n][Q].  x == NULL: the resident particles with their resident log-weights (M must equal the context's N,
 * logw must be NULL; nothing is uploaded); x != NULL with logw == NULL: equal weights.  Log-weights are unnormalised.  A
 * particle with a non-finite log-weight contributes to nothing, whatever its terms are; the others are "contributing".
 * Row 0 (header): [mw, sw, sw2, cnt, 0 ..] = the largest contributing log-weight (-inf: none), sum exp(lw - mw),
 * sum exp(2 (lw - mw)), the number of contributing particles.  Row 1 + i, observation i, with lw' = lw - mw, w = exp(lw')
 * and every sum over the contributing particles whose term ll is finite:
 *   0 ma    max (lw' + ll)                  (-inf: no such particle)
 *   1 Sa    sum exp(lw' + ll - ma)          lppd_i = ma + log Sa - log sw
 *   2 mb    max (lw' - ll)
 *   3 Sb    sum exp(lw' - ll - mb)          elpd_loo_i = -(mb + log Sb - log sw)
 *   4 Sb2   sum exp(2 (lw' - ll - mb))      loo_ess_i = Sb^2 / Sb2
 *   5 c     the first such particle's ll    (NaN: none) -- the shift of the two moments, inside the range of the terms
 *   6 SW    sum w
 *   7 S1    sum w (ll - c)                  mean_loglik_i = c + S1 / SW
 *   8 S2    sum w (ll - c)^2                p_waic_i = S2 / SW - (S1 / SW)^2  (never sum w ll^2 - mean^2)
 *   9 F     sum w E[y_i | x_p]              fitted_i = F / SW  (sigmoid(eta), e^eta, eta, e^eta for families 0..3)
 *  10 ninf  contributing particles with ll = -inf
 * Rules of the finished values (smcnuts_amd.criteria.combine_pointwise_partials): an observation with ninf > 0 has
 * lppd_i as defined (those particles add 0), mean_loglik_i = elpd_loo_i = -inf, loo_ess_i = 0 and p_waic_i, elpd_waic_i,
 * fitted_i NaN; all other observations are unaffected.  Every log-sum-exp is taken around its running maximum.
 * Merging two blocks (disjoint particle sets, in order): headers and the pairs (ma, Sa), (mb, Sb, Sb2) merge as max-shifted
 * sums after adding mw_k - max(mw) to ma / mb and scaling SW, S1, S2, F by exp(mw_k - max(mw)); the moments are re-centred
 * on the first block's c (d = c_2 - c: S1 += S1_2 + d SW_2, S2 += S2_2 + 2 d S1_2 + d^2 SW_2); ninf adds.  The result of one
 * call does not depend on the order in which its blocks finish (no atomics; the particle slices of a call follow from M
 * and n alone and are merged in slice order), so a repeated call returns identical bits.
 * smcn_pointwise_last_ms: the device time of the last smcn_pointwise_partials' kernels (HIP events on the context's
 * stream), for measurements. */
int smcn_pointwise_dims(const smcn_ctx* ctx, int64_t* n_obs, int* n_cols);
int smcn_pointwise_loglik(smcn_ctx* ctx, const double* x /* [M][D] */, int64_t M, double* out /* [M][n] */);
int smcn_pointwise_partials(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */,
                            int64_t M, double* out /* [1 + n][Q] */);
int smcn_pointwise_last_ms(const smcn_ctx* ctx, double* ms);

/* ---- calibration: predictive tails at the observations (SMCN_MODEL_GLM, all four families, D <= 64, any n) ----
 * Per particle x_p and observation i, with the predictive law family(eta_{p,i} [, e^tau_p]) -- eta and the dispersion as
 * the density forms them, o_i included:
 *   lo = P(Y < y_i),  up = P(Y > y_i),  pmf = P(Y = y_i) = exp(ll[p][i]) for the discrete families (normal: lo + up = 1)
 *   bernoulli_logit     lo: 0 (y = 0), sigmoid(-eta) (y = 1)            up: sigmoid(eta) (y = 0), 0 (y = 1)
 *   poisson_log         lo: Q(y, mu) (0 at y = 0)                       up: P(y + 1, mu)                mu = e^eta
 *   normal              lo: erfc(-z / sqrt 2) / 2                       up: erfc(z / sqrt 2) / 2        z = (y - eta) / sigma
 *   neg_binomial_2_log  lo: I_pr(phi, y) (0 at y = 0)                   up: I_{1 - pr}(y + 1, phi)      pr = phi / (mu + phi)
 * (P, Q: the regularised incomplete gamma functions; I: the regularised incomplete beta function).  Each tail has
 * relative accuracy: the smaller one is a series or continued fraction times pmf, the larger one 1 - pmf - the other.
 * Every such evaluation runs at most 2048 iterations; a pair that reaches the bound is "unconverged" (Poisson counts at
 * their mode need about 8 sqrt(mu): counts near 1e5 and beyond fall outside).  Served contexts and refusals: as
 * smcn_pointwise_* (SMCN_MODEL_GLM; SMCN_MODEL_OGLM with offsets alone; a weighted fit and every other model fail with a
 * message that says so).
 *
 * smcn_calibration_dims: n and the column count Qc (= 9) of a partials block.
 * smcn_calibration_points: out[M][n][2] = (lo, up) of every pair for M caller-supplied points x[M][D]; both NaN where
 * the term is not finite or the pair is unconverged.
 * smcn_calibration_partials: the sums OVER PARTICLES per observation as MERGEABLE partials out[1 + n][Qc]; x, logw, M,
 * "contributing" and row 0 (the header) exactly as smcn_pointwise_partials.  Row 1 + i, observation i, with
 * lw' = lw - mw, w = exp(lw') and every sum over the contributing particles whose term ll is finite and whose pair
 * converged:
 *   0 SW    sum w
 *   1 LO    sum w lo                        pit_lo_i = LO / SW
 *   2 UP    sum w up                        sf_i = UP / SW, pit_hi_i = 1 - sf_i
 *   3 mb    max (lw' - ll)                  (-inf: no such particle) -- the leave-one-out weights, smcn_pointwise_partials' mb
 *   4 Sb    sum exp(lw' - ll - mb)
 *   5 LOb   sum exp(lw' - ll - mb) lo       pit_lo_loo_i = LOb / Sb
 *   6 UPb   sum exp(lw' - ll - mb) up       sf_loo_i = UPb / Sb
 *   7 ninf  contributing particles with ll = -inf
 *   8 nunc  contributing particles whose pair is unconverged
 * Rules of the finished values (smcnuts_amd.calibration.combine_calibration_partials): an observation with ninf > 0 or
 * nunc > 0 reports NaN; all other observations are unaffected.
 * Merging two blocks (disjoint particle sets, in order): headers as smcn_pointwise_partials; SW, LO, UP are scaled by
 * exp(mw_k - max(mw)) and add; (mb, Sb, LOb, UPb) merge as max-shifted sums after adding mw_k - max(mw) to mb; ninf and
 * nunc add.  No atomics; the particle slices of a call follow from M and n alone and are merged in slice order, so a
 * repeated call returns identical bits.
 * smcn_calibration_last_ms: the device time of the last smcn_calibration_partials' kernels, for measurements. */
int smcn_calibration_dims(const smcn_ctx* ctx, int64_t* n_obs, int* n_cols);
int smcn_calibration_points(smcn_ctx* ctx, const double* x /* [M][D] */, int64_t M, double* out /* [M][n][2] */);
int smcn_calibration_partials(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */,
                              int64_t M, double* out /* [1 + n][Qc] */);
int smcn_calibration_last_ms(const smcn_ctx* ctx, double* ms);

/* ---- Pareto-smoothed importance-sampling LOO (SMCN_MODEL_GLM, all four families, D <= 64, any n) ----
 * PSIS-LOO of the weighted particles with the shape k of the fitted generalised Pareto tail as its diagnostic (definition:
 * DESIGN.md 4.4).  With lw' = lw - mw, ll = log p(y_i | x_p) and lr = lw' - ll over the contributing particles (finite
 * lw), S of them over all shards, mw the largest finite log-weight over all shards: M = min(S / 5, ceil(3 sqrt(S))) and
 * T_cap = M + 1.  Contexts of every other model fail with smcn_pointwise_*'s message.  Three stages, each a function of its
 * inputs and (mw, S) alone, and the single-rank wrapper; x == NULL takes the resident particles with their resident
 * log-weights (M = N, logw = NULL) as smcn_pointwise_partials does, logw == NULL with x means equal weights.
 *
 * smcn_psis_candidates: cand[2][n][T_cap] = per observation this rank's T_cap largest lr (first block) with their ll
 * (second block), descending in lr, equal lr in particle order, padded with -inf where the rank holds fewer.  The
 * selection is exact (radix selection by count on the bits of lr, then a sort on (lr, particle index)): the result depends
 * on the values alone.  T_cap <= 4096, i.e. S <= 1 863 225; larger S is refused with a message.
 * smcn_psis_body: body[n][4] = (mb, Sb, Sb2, Sw) over this rank's contributing particles with a finite term and
 * lr <= cutoff[i]: max lr, sum exp(lr - mb), sum exp(2 (lr - mb)), sum exp(lw').  Slices are merged in slice order; blocks
 * of disjoint particle sets merge as the (mb, Sb, Sb2) of smcn_pointwise_partials do, Sw adds.
 * smcn_psis_fit: from the merged candidates (T_cap per observation, any order) and merged body partials of n_obs
 * observations, out[n_obs][6] = pareto_k, elpd_psis, psis_ess, tail_len, cutoff, sigma.  mx is the largest candidate, c the
 * smallest minus mx, the tail the candidates with lr - mx > c (sorted on the device), cutoff the largest candidate that is
 * not in the tail (the value smcn_psis_body wants).  Fewer than 5 tail entries: pareto_k = +inf, sigma = NaN, nothing is
 * smoothed.  A candidate of +inf (a contributing particle with ll = -inf): pareto_k = +inf, elpd_psis = -inf, psis_ess = 0,
 * tail_len = 0, cutoff = +inf, sigma = NaN.  elpd_psis is log sum r~ p / sum r~ of the smoothed ratios (elpd_loo_i of
 * smcn_pointwise_partials with the tail replaced).  Needs no particles and no model: any n_obs, T_cap <= 4097.
 * smcn_psis_loo: the three stages back to back on one rank without a host round trip (mw and S are the call's own, formed
 * and read on the device); out[n][6], head_or_null[4] = smcn_pointwise_partials' header.  Bit for bit the staged calls.
 * smcn_psis_last_ms: ms[4] = device time of the last candidates, body, fit stage and of the last whole smcn_psis_loo (HIP
 * events on the context's stream), for measurements. */
int smcn_psis_candidates(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */,
                         int64_t M, double mw, int64_t S, double* cand /* [2][n][T_cap] */);
int smcn_psis_body(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */, int64_t M,
                   double mw, int64_t S, const double* cutoff /* [n] */, double* body /* [n][4] */);
int smcn_psis_fit(smcn_ctx* ctx, const double* cand /* [2][n_obs][T_cap] */, const double* body /* [n_obs][4] */,
                  int64_t n_obs, double mw, int64_t S, double* out /* [n_obs][6] */);
int smcn_psis_loo(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */, int64_t M,
                  double* out /* [n][6] */, double* head_or_null /* [4] */);
int smcn_psis_last_ms(const smcn_ctx* ctx, double* ms /* [4] */);

/* ---- held-out prediction at new rows (SMCN_MODEL_GLM, SMCN_MODEL_OGLM, SMCN_MODEL_HGLM, SMCN_MODEL_CATEGORICAL,
 * SMCN_MODEL_ORDINAL) ----
 * Posterior predictive summaries at rows the model was not fitted to, and log p(y_new_i | x_p) when y_new is given.
 * Contexts of every other model (arma, PRMwCD, Gaussian, host-evaluated) fail with a message that names these.
 *
 * smcn_predict_set_data: the new rows, as the model's own data block WITHOUT the priors:
 *   SMCN_MODEL_GLM          [family, m, p, intercept, y_1..y_m, X (m x p, row-major)]
 *   SMCN_MODEL_OGLM         [family, m, p, intercept, flags, y_1..y_m, o_1..o_m (flags & 1), w_1..w_m = 1 (flags & 2), X]
 *                           (the new rows' own offsets; their weights are not read: a term is log p(y_i | x))
 *   SMCN_MODEL_HGLM         [family, m, p, intercept, J, y_1..y_m, g_1..g_m, X]     (g: existing groups 0..J-1 only)
 *   SMCN_MODEL_CATEGORICAL  [K, m, p, intercept, y_1..y_m, X]
 *   SMCN_MODEL_ORDINAL      [K, m, p, y_1..y_m, X]
 * Every header entry but m must repeat the training block's.  has_y = 0: the y slots hold zeros and the lpd columns of
 * the partials are meaningless (smcn_predict_loglik refuses).  The block is validated by the rules of smcn_ctx_create
 * (finite X, labels in 0..K-1, y in {0, 1} / counts, g in 0..J-1) and repacked into the padded row table by the routine
 * that repacks the training design.  The table is owned by the context and replaced by the next call.
 * smcn_predict_dims: m, the column count Q of a partials block and has_y.
 * smcn_predict_loglik: log p(y_new_i | x_p) as [M][m] row-major for M caller-supplied points (the plain form).  At the
 * training rows its row sums are the llik of smcn_target_eval.
 * smcn_predict_partials: MERGEABLE partials out[1 + m][Q]; x == NULL: the resident particles with their resident
 * log-weights (M = N, logw = NULL), as smcn_pointwise_partials.  Row 0 is smcn_pointwise_partials' header
 * [mw, sw, sw2, cnt, 0 ..].  Row 1 + i, new row i, with lw' = lw - mw, w = exp(lw'), over the contributing particles:
 *   0 ma    max (lw' + ll) over finite ll      (-inf: none)
 *   1 Sa    sum exp(lw' + ll - ma)             lpd_i = ma + log Sa - log sw
 *   2 ninf  particles with ll = -inf (they add 0 to lpd_i)
 *   3 nbad  particles with a non-finite predictive mean, variance or probability: the row's summaries are NaN
 *  GLM families and hierarchical (Q = 9), sums over the particles that nbad does not count, mu_p = E[y_i | x_p]:
 *   4 c     the first such mu_p (NaN: none)    the shift of the moments
 *   5 SW    sum w
 *   6 S1    sum w (mu_p - c)                   mean_i = c + S1 / SW
 *   7 S2    sum w (mu_p - c)^2                 between-particle variance S2 / SW - (S1 / SW)^2 (never sum w mu^2 - mean^2)
 *   8 V     sum w Var(y_i | x_p)               var_i = V / SW + the between-particle variance
 *           (Var: p (1 - p), mu, sigma^2, mu + mu^2 / phi for families 0..3)
 *  categorical (Q = 4 + K):
 *   4 + k   sum w P(y_i = k | x_p), k = 0..K-1          prob[i][k] = that / sw
 *  ordinal (Q = 5 + K for K <= 16, Q = 5 above):
 *   4 EM    sum w sum_k sigma(eta_i - c_k)              mean_i (expected class index) = EM / sw
 *   5 + k   sum w P(y_i = k | x_p)                      (K <= 16 only)
 * Merging two blocks (disjoint particle sets, in order) follows smcn_pointwise_partials: headers and (ma, Sa) as
 * max-shifted sums, the moments re-centred on the first block's c, every other column scaled by exp(mw_k - max(mw)) and
 * added; ninf and nbad add unscaled.  The particle slices of a call follow from (M, m) alone and are merged in slice order
 * (no atomics): a repeated call returns identical bits.
 * smcn_predict_last_ms: the device time of the last smcn_predict_partials' kernels. */
int smcn_predict_set_data(smcn_ctx* ctx, const double* block, int64_t len, int has_y);
int smcn_predict_dims(smcn_ctx* ctx, int64_t* n_rows, int* n_cols, int* has_y);
int smcn_predict_loglik(smcn_ctx* ctx, const double* x /* [M][D] */, int64_t M, double* out /* [M][m] */);
int smcn_predict_partials(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */,
                          int64_t M, double* out /* [1 + m][Q] */);
int smcn_predict_last_ms(const smcn_ctx* ctx, double* ms);

/* ---- posterior predictive draws at the rows of the last smcn_predict_set_data (the same four models) ----
 * smcn_predict_draws: y_out[j][i] ~ p(. | x_{a_s}, row i) for the slots s = s_first + j, j < s_count, of S: draw s is ONE
 * replicated data set of the m rows from ONE ancestor particle a_s.  x == NULL: the resident particles with their
 * resident log-weights (M = N, logw = NULL); logw == NULL with x: equal weights.
 * Ancestors: systematic resampling with S slots.  W the normalised weights in particle order, C their inclusive
 * cumulative sum, u0 = philox_uniform(seed, iter 0, particle 0, stream 16, q 0), a_s = min{p : C_p > (s + u0) / S},
 * clamped to the last particle with a finite log-weight; a particle with a non-finite log-weight is never chosen.
 * ancestors != NULL ([S], each in 0..M-1) replaces them: the way to draw from chosen particles.
 * Uniforms: philox_uniform(seed, iter = s, particle = i (the row), stream, q) with streams 17 outcome, 18 gamma,
 * 19 new-group intercept (particle = the group's label): a draw depends on (seed, s, i) and its ancestor alone, not on
 * the slot range, the tiling or S.
 * Samplers: Bernoulli [u < p]; categorical min{k : P_0 + .. + P_k > u}, else K - 1; ordinal #{k : c_k < eta + log u -
 * log1p(-u)}; normal eta + sigma z, z = sqrt(-2 log1p(-u_0)) cos(2 pi u_1); Poisson by inversion below mu = 10 (at most
 * 1000 steps) and by Hoermann's PTRS from 10 (attempt t: uniforms 2t, 2t + 1); NB2 as Poisson(mu G / phi) with
 * G ~ Gamma(phi, 1) by Marsaglia-Tsang on stream 18 (attempt t: uniforms 3t, 3t + 1 (Box-Muller), 3t + 2; phi < 1: shape
 * phi + 1 and the boost u_192^(1 / phi)); 64 attempts at most.  Above mu of about 1e15 the rounding grid of the doubles
 * shows in the variance of the PTRS draws.
 * SMCN_MODEL_HGLM: new_group != NULL ([m]) gives per row the label of a NEW group (>= J; rows that share a label share
 * the group) or any value below J for a row of the fitted group the block names; a new group's intercept is tau_p z,
 * z the Box-Muller cosine of stream 19 at (iter = s, particle = label, q = 0, 1).  Rows of new groups carry group 0 in
 * the block.  NULL for every other model.
 * Bad draws are NaN and counted in *n_bad_out: a non-finite eta, logit (-inf included), mean or cutpoint, mu > 2^53, a
 * dispersion coordinate the density refuses, e^eta or e^(2 lt) overflowing, an attempt cap reached.
 * smcn_predict_draws_last_ms: the device time of the last smcn_predict_draws' kernels. */
int smcn_predict_draws(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */, int64_t M,
                       int64_t S, uint64_t seed, const int64_t* ancestors_or_null /* [S] */,
                       const int64_t* new_group_or_null /* [m] */, int64_t s_first, int64_t s_count,
                       double* y_out /* [s_count][m] */, int64_t* ancestors_out /* [s_count] */, int64_t* n_bad_out);
int smcn_predict_draws_last_ms(const smcn_ctx* ctx, double* ms);

/* ---- posterior summaries: weighted quantiles and tail masses of the constrained coordinates (every model) ----
 * Definition.  For a constrained coordinate with values v_i and weights w_i >= 0 of total W, and p in (0, 1]:
 *   Q(p) = min { v_j : sum over {i : v_i <= v_j} of w_i >= p W }     (the inverse of the weighted empirical CDF)
 *   F(t) = (sum over {i : v_i <= t} of w_i) / W
 * A quantile is one of the particles' own values.  Particles of zero weight never contribute; +-inf sort at the ends;
 * -0.0 and +0.0 are equal; a NaN in a particle of positive weight is reported by a flag per coordinate.
 * Masses are integers: w_i / W is converted once to units of 2^-52 (rounded to nearest, at least one unit for a positive
 * weight), and every sum is an unsigned 64-bit integer sum -- exact in any order, below 2^53 for any population, so also
 * exact as the doubles these entry points return.  A result therefore depends on the multiset of (value, weight) pairs
 * alone: not on the order of the particles or the launch geometry; every shard of a run returns the same bits.
 * Selection is a radix select on the order-preserving key of a double (non-negative: sign bit flipped; negative: all
 * bits inverted), most significant byte first: 8 passes, digit k of a key being its byte 7 - k.
 *
 * smcn_summary_begin stages a population: x == v == NULL the resident particles and log-weights (M = N, logw = NULL)
 * through the model's constrain path; x [M][D] unconstrained points through the same path; v [M][Dv] values that are
 * already constrained (host-evaluated targets).  logw == NULL with x or v: equal weights.  head_out: [largest finite
 * log-weight mw, sum exp(lw - mw), sum exp(2 (lw - mw)), particles with a finite log-weight] of THIS shard.
 * smcn_summary_weights converts the staged log-weights against the maximum and the total of ALL shards (one shard: head_out's
 * own; several: mw = max_r mw_r, sum = sum_r s_r exp(mw_r - mw)) and returns this shard's mass in units.
 * One shard: smcn_summary_select runs the eight passes on the device with one wait at the end.  thresholds[q] =
 * ceil(p_q * total mass), ascending, the same for every coordinate.
 * Several shards: per pass k = 0..7, smcn_summary_hist returns this shard's histograms, out[Dc][nl][256] doubles with
 * nl = 1 in pass 0 (no prefix: shared by the probabilities) and nl = nq after, followed by the Dc NaN flags; the caller
 * sums them over the shards, takes per (coordinate, probability) the first digit whose cumulative mass reaches the
 * remaining threshold, and hands every shard the same digits and the thresholds less the mass below the digit
 * (smcn_summary_descend, [Dc][nq] each).  Probabilities in ascending order.
 * smcn_summary_values: the selected values out[Dc][nq] after the eighth pass and the Dc NaN flags of this shard.
 * smcn_summary_cdf: this shard's mass at or below at[c][j], out[Dc][T] in units, followed by the Dc NaN flags.
 * smcn_summary_last_ms: device time of the kernels since the last smcn_summary_begin (HIP events on the context's
 * stream); smcn_summary_pass_ms: of each of the eight passes of the last selection (histogram and pick). */
int smcn_summary_begin(smcn_ctx* ctx, const double* x_or_null /* [M][D] */, const double* logw_or_null /* [M] */,
                       const double* v_or_null /* [M][Dv] */, int64_t M, int Dv, double* head_out /* [4] */);
int smcn_summary_weights(smcn_ctx* ctx, double lw_max, double lw_sum, double* mass_out);
int smcn_summary_select(smcn_ctx* ctx, int nq, const double* thresholds /* [nq] */);
int smcn_summary_hist(smcn_ctx* ctx, int pass, int nq, double* out /* [Dc][nl][256] + [Dc] */);
int smcn_summary_descend(smcn_ctx* ctx, int pass, int nq, const int32_t* digits /* [Dc][nq] */,
                         const double* residual /* [Dc][nq] */);
int smcn_summary_values(smcn_ctx* ctx, int nq, double* out /* [Dc][nq] */, double* nan_flags_out /* [Dc] */);
int smcn_summary_cdf(smcn_ctx* ctx, int T, const double* at /* [Dc][T] */, double* out /* [Dc][T] + [Dc] */);
int smcn_summary_last_ms(const smcn_ctx* ctx, double* ms);
int smcn_summary_pass_ms(const smcn_ctx* ctx, double* ms /* [8] */);

/* ---- posterior covariance: weighted second moments of the constrained coordinates (every model) ----
 * Definition.  Over the particles with a finite log-weight, w_p = exp(lw_p - mw) (mw: the largest finite log-weight of
 * ALL shards), W = sum w_p, v_p the constrained vector (Dc values):
 *   m_i = sum w_p v_ip / W        C_ij = sum w_p (v_ip - m_i)(v_jp - m_j) / W       (weights normalised to one, no
 * small-sample correction: diag C is the variance estimate).  A particle of weight 0 contributes nothing and its values
 * are never multiplied; a non-finite value in a particle of positive weight reaches row and column i alone.
 * The device never forms sum w v v^T - m m^T.  It sums about a centre c near the mean,
 *   G_ij = sum w_p (v_ip - c_i)(v_jp - c_j),   S1_i = sum w_p (v_ip - c_i),   W,
 * as one symmetric product of the population with one constant coordinate "1" appended (fp64 MFMA, smcn_cov.hpp), and
 * the caller finishes: d = S1 / W, C = G / W - d d^T, m = c + d.  Partials of disjoint sets of particles with the same
 * centre and the same mw add.
 *
 * smcn_cov_partials runs on the population staged by the last smcn_summary_begin (resident, x, or v).  lw_max: mw.
 * centre [Dc], or NULL: the shard's own weighted mean (0 where the shard has no weight).  slices: particle slices of the
 * launch, 0 for the rule's own count (a function of M and Dc alone; smcn_cov_dims) or 1 .. the cap -- the slices'
 * partials stay below 64 MiB and 1024 slices.  A result depends on (population, lw_max, centre, slices) alone: slices
 * are merged per entry in slice order, 16 at a time and then the groups, with no atomics.  out [Dc+1][Dc+1]: the
 * symmetric augmented matrix [[G, S1], [S1^T, W]], un-normalised; NULL: only the centre is formed.  centre_out [Dc]
 * (or NULL): the centre used.  Dc <= 1023.
 * smcn_cov_dims: out[4] = {M, Dc, the rule's slices, the cap} of the staged population (the last two 0 for Dc > 1023).
 * smcn_cov_last_ms: device time of the last smcn_cov_partials' kernels (HIP events on the context's stream). */
int smcn_cov_partials(smcn_ctx* ctx, double lw_max, const double* centre_or_null /* [Dc] */, int64_t slices,
                      double* out /* [Dc+1][Dc+1] */, double* centre_out /* [Dc] */);
int smcn_cov_dims(const smcn_ctx* ctx, int64_t* out /* [4] */);
int smcn_cov_last_ms(const smcn_ctx* ctx, double* ms);

/* ---- step-size probe: short leapfrog trajectories at a ladder of step sizes (every device-native model) ----
 * x [M][D] with logw [M] (NULL: equal), or x = NULL: the resident particles with their resident log-weights (logw = NULL,
 * M = N).  Mp = min(M, max_particles) particles are probed, probed particle k being particle (k M) / Mp.  Momenta: r
 * [Mp][D], or NULL: standard normal draws, Philox keyed by (coordinate pair, particle_base + particle, 0, a stream no
 * sampler kernel draws from) under `seed`, the Box-Muller of the sampler's momentum draw -- a function of (seed, global
 * particle index) alone.
 * Per probed particle and ladder entry j (1 <= L <= 16; finite, positive, strictly increasing) the trajectory restarts
 * from the same (x, r) and runs n_leapfrog (1 .. 64) steps of size eps_j on log pi_phi = lpri + phi llik:
 *   r += eps/2 g;  x += eps r;  g = grad log pi_phi(x);  r += eps/2 g;  dH_t = H_t - H_0,  H = -log pi_phi + |r|^2 / 2
 *   a_j = (1/n) sum_t min(1, exp(-dH_t)).
 * The first t at which dH_t is not finite or exceeds delta_max marks the pair divergent: that step and all later ones
 * contribute 0 (first_bad = t, else 0).  A particle whose starting density or log-weight is not finite is excluded
 * (a = 0, first_bad = 0) and counted.
 * partials [1 + L][4]: row 0 = (m, Mp, excluded, 0), m the largest finite log-weight probed (-inf: none); row 1 + j =
 * (sum w a_j, sum w d_j, sum w, number divergent) over the particles that count, w = exp(logw - m), d_j the divergent
 * flag.  Summed in a fixed order without atomics: two calls give the same bits.  Partials of disjoint particle sets
 * merge after rescaling by exp(m_r - m).  accept, first_bad [L][Mp] (or NULL): the per-particle values.
 * The call reads the resident particles and weights and writes buffers of its own and the staging buffer: the sampler's
 * state, momenta, flags, history and block buffers stay as they were.  SMCN_MODEL_HOST is refused.
 * smcn_stepsize_last_ms: device time of the last probe's kernels (HIP events on the context's stream); -1: no context. */
int smcn_stepsize_probe(smcn_ctx* ctx, const double* x, const double* logw, int64_t M, const double* r,
                        const double* ladder, int L, int n_leapfrog, double phi, double delta_max, uint64_t seed,
                        int64_t max_particles, double* partials /* [1 + L][4] */, double* accept /* [L][Mp] or NULL */,
                        int32_t* first_bad /* [L][Mp] or NULL */);
double smcn_stepsize_last_ms(const smcn_ctx* ctx);

/* ---- forecasts of the arma target (SMCN_MODEL_ARMA only; every other model fails with a message that names it) ----
 * Per point x = (mu, beta, theta, s), sigma = exp(s), and the context's series y_1..y_T (y_0 := mu, err_0 := 0):
 *   err_1 = fma(-beta, mu, y_1 - mu),  err_t = fma(-theta, err_{t-1}, fma(-beta, y_{t-1}, y_t - mu))   (the density's bits)
 *   y_{T+h} | y_{1:T}, x ~ N(m_h, v_h):  m_1 = fma(theta, err_T, fma(beta, y_T, mu)),  m_h = fma(beta, m_{h-1}, mu);
 *   psi_0 = 1, psi_1 = beta + theta, psi_j = beta psi_{j-1};  C_1 = 1, C_h = fma(psi_{h-1}, psi_{h-1}, C_{h-1});
 *   v_h = (sigma sigma) C_h.   Iterative: no 1 / (1 - beta); |beta| >= 1 gives growing, finite variances.
 * A point is BAD at h when sigma, m_h or v_h is not finite or v_h <= 0.
 * With a held-out continuation yf_1..yf_H:
 *   marginal term  a_h = -0.5 (log 2 pi + log v_h) - 0.5 (yf_h - m_h)^2 / v_h      (NaN when bad at h)
 *   joint term     J_h = sum_{j<=h} l_j,  l_j = (-0.5 log 2 pi - s) - 0.5 (e_j / sigma)^2, the recurrence continued through
 *                  the held-out values: e_j = fma(-theta, e_{j-1}, fma(-beta, yf_{j-1}, yf_j - mu)), yf_0 = y_T, e_0 = err_T;
 *                  J_h = llik(y_{1:T}, yf_{1:h}) - llik(y_{1:T}) of the arma density.
 *
 * smcn_forecast_set: the horizon H (1..512), the continuation y_future [H] or NULL, and thresholds at [H][Tn] (Tn 0..16,
 * NULL with Tn = 0); all finite.  Owned by the context, replaced by the next call.
 * smcn_forecast_dims: H, the column count Q = 10 + Tn of a partials block, whether y_future was given, Tn.
 * smcn_forecast_slices: the particle slices of a smcn_forecast_partials call over M particles (a function of M alone:
 * blocks of 256 particles), merged in slice order.
 * smcn_forecast_points: the plain form for M caller-supplied points, out[M][W] row-major, W = 1 + 2H, with y_future
 * 1 + 4H: err_T, m_1..m_H, v_1..v_H (, a_1..a_H, J_1..J_H).  A row with a non-finite coordinate is NaN throughout.
 * smcn_forecast_partials: MERGEABLE partials out[1 + H][Q]; x == NULL: the resident particles with their resident
 * log-weights (M = N, logw = NULL); logw == NULL with x: equal weights.  Row 0 is smcn_pointwise_partials' header
 * [mw, sw, sw2, cnt, 0 ..].  Row h, with lw' = lw - mw, w = exp(lw'), over the contributing particles (finite lw) that are
 * not bad at h:
 *   0 ma    max (lw' + a_h) over finite terms  (-inf: none)
 *   1 Sa    sum exp(lw' + a_h - ma)            lpd_marginal_h = ma + log Sa - log sw
 *   2 mj    max (lw' + J_h) over finite terms
 *   3 Sj    sum exp(lw' + J_h - mj)            lpd_joint_h = mj + log Sj - log sw
 *   4 nbad  contributing particles that are bad at h: the row's moments and cdf are NaN
 *   5 c     the shift of the moments (NaN: none): a wavefront's weighted mean of m_h, formed about the m_h of its first such
 *           particle with w > 0; merged blocks keep the first block's
 *   6 SW    sum w
 *   7 S1    sum w (m_h - c)                    mean_h = c + S1 / SW
 *   8 S2    sum w (m_h - c)^2                  between-particle variance S2 / SW - (S1 / SW)^2 (never sum w m^2 - mean^2)
 *   9 V     sum w v_h                          var_h = V / SW + the between-particle variance
 *   10 + k  sum w Phi((at[h][k] - m_h) / sqrt(v_h))      cdf[h][k] = that / SW
 * Without y_future columns 0..3 are (-inf, 0, -inf, 0).  Merging two blocks (disjoint particle sets, in order) follows
 * smcn_predict_partials: headers and the two (max, sum) pairs as max-shifted sums, the moments re-centred on the first
 * block's c, every other column scaled by exp(mw_k - max(mw)) and added; nbad adds unscaled.  No atomics: a repeated call
 * returns identical bits.
 * smcn_forecast_draws: y_out[j][h - 1] = y_{T+h} of the path of slot s = s_first + j, j < s_count, of S, simulated from
 * ONE particle a_s.  Ancestors: smcn_predict_draws' systematic rule with u0 = philox_uniform(seed, 0, 0, stream 20, 0);
 * ancestors != NULL ([S], each in 0..M-1) replaces them.  z_{s,h} = sqrt(-2 log1p(-u_0)) cos(2 pi u_1), (u_0, u_1) the
 * uniforms q = 0, 1 of philox_uniform(seed, iter = s, particle = h, stream 21), h = 1..H; e_h = sigma z_{s,h};
 *   y_{T+1} = m_1 + e_1,   y_{T+h} = fma(theta, e_{h-1}, fma(beta, y_{T+h-1}, mu)) + e_h.
 * A value depends on (seed, s, h) and its ancestor alone: not on S, the slot range or the tiling.  From the first
 * non-finite value on a path is NaN; *n_bad_out counts the NaN values.
 * smcn_forecast_last_ms: device time of the kernels of the last smcn_forecast_partials (ms[0]) and smcn_forecast_draws
 * (ms[1]) (HIP events on the context's stream). */
int smcn_forecast_set(smcn_ctx* ctx, int64_t H, const double* y_future_or_null /* [H] */,
                      const double* at_or_null /* [H][Tn] */, int Tn);
int smcn_forecast_dims(smcn_ctx* ctx, int64_t* H, int* Q, int* has_y, int* Tn);
int smcn_forecast_slices(smcn_ctx* ctx, int64_t M, int64_t* slices);
int smcn_forecast_points(smcn_ctx* ctx, const double* x /* [M][4] */, int64_t M, double* out /* [M][W] */);
int smcn_forecast_partials(smcn_ctx* ctx, const double* x_or_null /* [M][4] */, const double* logw_or_null /* [M] */,
                           int64_t M, double* out /* [1 + H][Q] */);
int smcn_forecast_draws(smcn_ctx* ctx, const double* x_or_null /* [M][4] */, const double* logw_or_null /* [M] */, int64_t M,
                        int64_t S, uint64_t seed, const int64_t* ancestors_or_null /* [S] */, int64_t s_first,
                        int64_t s_count, double* y_out /* [s_count][H] */, int64_t* ancestors_out /* [s_count] */,
                        int64_t* n_bad_out);
int smcn_forecast_last_ms(const smcn_ctx* ctx, double ms[2]);

/* ---- one-step residual checks of the arma target (SMCN_MODEL_ARMA only; every other model fails with a message that
 * names it).  Per point x = (mu, beta, theta, s), sigma = exp(s), and the context's series y_1..y_T, in this operation order:
 *   err_t as above (the density's bits: err_T is what smcn_forecast_points reports)
 *   nu_t = y_t - err_t                                   the one-step mean
 *   r_t = err_t / sigma                                  the standardised residual
 *   l_t = (-0.5 log 2 pi - s) - 0.5 (r_t r_t)            the one-step term; sum_t l_t is the arma log-likelihood
 *   PIT_t = Phi(r_t) = 0.5 erfc(-r_t sqrt(1/2))
 * A point is BAD at t when sigma is not finite or not > 0, or err_t or r_t is not finite.  A point whose err_t or r_t is
 * finite but whose square is not (beyond about 1e154: a chain on its way to overflowing) is NOT bad at t: that row's second
 * moments (S2, Z2: var and z_sd) are then inf or NaN while its bad count is still 0.
 * With L lags (0..32, L <= T - 1), r_t := 0 for t < 1, all sums from 0 in ascending t:
 *   A_0 = fma(r_t, r_t, A_0),  A_k = fma(r_t, r_{t-k}, A_k);   rho_k = A_k / A_0   (uncentred)
 *   Q = (T (T + 2)) sum_{k=1..L} (rho_k rho_k) / (T - k)       (ascending k)
 * A point is BAD FOR THE LAG ROWS when it is bad at any t, or A_0 is not finite or not > 0, or Q is not finite.  Q is the
 * Ljung-Box statistic of the residuals REALISED at x: at a draw from the posterior the r_t are iid N(0, 1) if the model
 * holds, so Q is compared with chi-square on L degrees of freedom, with no correction for the fitted parameters.
 *
 * smcn_residuals_set: the lags L and thresholds q_at [Tn] of Q (Tn 0..8, NULL with Tn = 0, only with L >= 1); all finite.
 * Series with (T + L + 2) * 20 > 2^18 are refused.  Owned by the context, replaced by the next call.
 * smcn_residuals_dims: T, L, the column count Qc = 20 of a partials block, Tn.
 * smcn_residuals_points: the plain form for M caller-supplied points, out[M][W] row-major, W = 2T + (L > 0 ? L + 1 : 0):
 * nu_1..nu_T, r_1..r_T (, rho_1..rho_L, Q).  A row with a non-finite coordinate is NaN throughout.
 * smcn_residuals_partials: MERGEABLE partials out[1 + T + (L > 0 ? L + 1 : 0)][20]; x == NULL: the resident particles with
 * their resident log-weights (M = N, logw = NULL); logw == NULL with x: equal weights.  Row 0 is smcn_pointwise_partials'
 * header [mw, sw, sw2, cnt, 0 ..].  Time row t (row t), with lw' = lw - mw, w = exp(lw'), over the contributing particles
 * (finite lw) that are not bad at t:
 *   0 ml    max (lw' + l_t) over finite terms  (-inf: none)
 *   1 Sl    sum exp(lw' + l_t - ml)            lpd_t = ml + log Sl - log sw
 *   2 nbad  contributing particles that are bad at t: the row's moments, z and pit are NaN
 *   3 c     the shift of nu_t's moments (NaN: none): a wavefront's weighted mean, formed about the nu_t of its first such
 *           particle with w > 0; merged blocks keep the first block's
 *   4 SW    sum w
 *   5 S1    sum w (nu_t - c)                   mean_t = c + S1 / SW
 *   6 S2    sum w (nu_t - c)^2                 between-particle variance S2 / SW - (S1 / SW)^2
 *   7 V     sum w sigma^2                      var_t = V / SW + the between-particle variance
 *   8 cz    the shift of r_t's moments, formed in the same way
 *   9 Z1    sum w (r_t - cz)                   z_t = cz + Z1 / SW
 *   10 Z2   sum w (r_t - cz)^2                 z_sd_t^2 = Z2 / SW - (Z1 / SW)^2  (never sum w r^2 - mean^2)
 *   11 U    sum w Phi(r_t)                     pit_t = U / SW
 *   12..19  0
 * Lag row k (row T + k, k = 1..L) and the Q row (row T + L + 1), present with L > 0, over the contributing particles that
 * are not bad for the lag rows: column 2 counts the contributing particles that are; columns 3..6 are c, SW, S1, S2 of
 * rho_k (of Q); columns 0, 1 are (-inf, 0), columns 8..10 (NaN, 0, 0), column 7 and 11 are 0.  The Q row's column 12 + j
 * is sum w [Q > q_at[j]], j < Tn; every other column from 12 on is 0.
 * Merging two blocks (disjoint particle sets, in order) follows smcn_forecast_partials: headers and (ml, Sl) as
 * max-shifted sums, the two moment groups re-centred on the first block's shifts, column 2 added unscaled, every other
 * column scaled by exp(mw_k - max(mw)) and added.  The slices (blocks of 256 particles, a function of M alone) are merged
 * in slice order, 16 at a time and then the groups.  No atomics: a repeated call returns identical bits.
 * smcn_residuals_last_ms: device time of the kernels of the last smcn_residuals_partials (HIP events on the context's
 * stream). */
int smcn_residuals_set(smcn_ctx* ctx, int L, const double* q_at_or_null /* [Tn] */, int Tn);
int smcn_residuals_dims(smcn_ctx* ctx, int64_t* T, int* L, int* Qc, int* Tn);
int smcn_residuals_points(smcn_ctx* ctx, const double* x /* [M][4] */, int64_t M, double* out /* [M][W] */);
int smcn_residuals_partials(smcn_ctx* ctx, const double* x_or_null /* [M][4] */, const double* logw_or_null /* [M] */,
                            int64_t M, double* out /* [1 + T + (L > 0 ? L + 1 : 0)][20] */);
int smcn_residuals_last_ms(const smcn_ctx* ctx, double* ms);

/* Diagnostic builds only (-DSMCN_PROFILE): in-kernel cycle sums per section of
 * the NUTS loop, summed over wavefronts (out[0..7]; out[8], out[9]: loop trips of all wavefronts
 * and of the longest one); zeros in a normal build.  With -DSMCN_PROFILE_PHASE as well the lane kernel's slots are by the
 * iteration's number mod 4 instead (csrc/smcn_nuts.hpp; tools/prof_sections.py with PROF_PHASE=1 prints them).
 * `reset`: bit 0 clears the sums after the read; bit 1 reads the second page of 16 slots (the phase build's cycles of the
 * in-phase iterations) instead of the first. */
int smcn_debug_profile(smcn_ctx* ctx, uint64_t out[16], int reset);

#ifdef __cplusplus
}
#endif
#endif
