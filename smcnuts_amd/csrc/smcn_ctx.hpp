// What the units of libsmcnuts_hip.so share (internal, not installed): the context, its owner types, the entry points'
// macros and the few host helpers that cross units.  smcn_api.hip is the core (context, sampler, loops, exchange); the
// post-fit subsystems are smcn_loo.hip, smcn_predict.hip, smcn_summary.hip and smcn_forecast.hip (forecasts and the
// one-step residual checks), each with its own sub-structs of smcn_ctx.
// Every __global__ function is instantiated in exactly ONE unit: a unit that needs another's kernel calls the host
// launcher declared at the end of this file.  Everything here but smcn_ctx lives in smcn_host, whose symbols are hidden:
// none of them reaches the library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/smcnuts_hip.h"
#include "smcn_comm.hpp"
#include "smcn_devbuf.hpp"
#include "smcn_draw_plan.hpp"
#include "smcn_regdata.hpp"

namespace smcn { struct PwArgs; }   // (smcn_pw_walk.hpp)

namespace smcn_host __attribute__((visibility("hidden"))) {
using namespace smcn;
constexpr int kTimerRing = 512;   // NUTS launches timed between two smcn_timers calls

// What a context owns on the device (smcn_devbuf.hpp): buffers from the core's per-device cache, pinned host memory, events
struct CacheMem { static int alloc(void** p, size_t bytes); static void free(void* p, bool synced); };
struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes); }
    static void free(void* p, bool) { (void)hipHostFree(p); }
};
struct HipEv {
    using event = hipEvent_t;
    using stream = hipStream_t;
    static int create(event* e, bool timing) { return (int)(timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming)); }
    static int record(event e, stream s) { return (int)hipEventRecord(e, s); }
    static int wait(event e) { return (int)hipEventSynchronize(e); }
    static int elapsed(float* ms, event from, event to) { return (int)hipEventElapsedTime(ms, from, to); }
    static void destroy(event e) { (void)hipEventDestroy(e); }
};
template <class T>
using Buf = DevBuf<T, CacheMem>;
using Event = DevEvent<HipEv>;

// pointwise criteria (smcn_pointwise_*): log-weights, slice partials and the result of a call; its kernels' time
struct PwState {
    Buf<double> buf;
    Event ev0, ev1;     // (around the kernels of smcn_predict_partials and smcn_predict_draws too)
    double ms = 0.0;
    double cal_ms = 0.0;   // smcn_calibration_partials' kernels (they use buf and the events as well)
};
// Pareto-smoothed LOO (smcn_psis_*): header, log-weights, the staged slab of ll, candidates, cutoffs, body partials and
// the result of a call; device time of the stages of the last calls (candidates, body, fit, whole smcn_psis_loo)
struct PsState {
    Buf<double> buf;
    Event ev[4];
    double ms[4] = {};
};
// held-out prediction (smcn_predict_*): the new rows' image [block | padding | table] as smcn_ctx_create lays out the
// training data, its layout (lay.n new rows, 0: none set) and whether they came with y
struct PrState {
    Buf<double> md;
    RegLayout lay;
    int has_y = 0;
    double ms = 0.0;
};
// posterior predictive draws (smcn_predict_draws): weights, scan, ancestors, gathered particles and the draws of a call
struct DrState {
    Buf<double> buf;
    double ms = 0.0;
};
// posterior summaries (smcn_summary_*): the staged population of a call (constrained values, fixed-point weights,
// selection state), its histograms, and the device time of its kernels
struct SmState {
    Buf<double> buf;
    Buf<unsigned long long> hist;
    int64_t M = 0;
    int Dc = 0, cur = 0, stage_state = 0;    // (state: 0 nothing staged, 1 values, 2 values and weights)
    std::vector<unsigned long long> pfx_h, thr_h;
    Event ev[10];
    double ms = 0.0, pass_ms[8] = {};
};
// posterior covariance (smcn_cov_*): weights, centre, slice and group partials, result
struct CovState {
    Buf<double> buf;
    Event ev[2];
    double ms = 0.0;
};
// step-size probe (smcn_stepsize_probe): staged log-weights and momenta, a [L][Mp], the partials; first-bad steps and
// excluded flags; its kernels' time.  Its own buffers: the probe leaves every resident one as it found it
struct StState {
    Buf<double> buf;
    Buf<int32_t> ibuf;
    Event ev0, ev1;
    double ms = 0.0;
};
// arma forecasts (smcn_forecast_*): the setting of the last smcn_forecast_set ([y_future H | at H Tn] on the device, H = 0:
// none), the slices' and groups' partials and the result of a call, the paths' work area; device time of the last
// partials and draws calls
struct FcState {
    Buf<double> set, buf, dbuf;
    int64_t H = 0;
    int Tn = 0, has_y = 0;
    Event ev0, ev1;
    double ms[2] = {};
};
// one-step residual checks of the arma target (smcn_residuals_*): the setting of the last smcn_residuals_set (L lags, -1:
// none; the Tn thresholds of Q on the device), the log-weights, slices' and groups' partials and the result of a call;
// device time of the last partials call
struct RsState {
    Buf<double> set, buf;
    int L = -1, Tn = 0;
    Event ev0, ev1;
    double ms = 0.0;
};
}  // namespace smcn_host
using namespace smcn_host;

struct smcn_ctx {
    int device = 0;
    int64_t N = 0, base = 0;
    int model = 0, D = 0, Dc = 0;
    int cmodel = 0;   // the model id the constrained-space kernels get (constrain_coord: ids 1 and 2 exp the last coordinate)
    int num_cu = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t seed = 0;
    std::string err;
    std::vector<double> mdata_h;
    RegLayout reg;              // the regression models: where things sit in mdata_h and in its image mdata (smcn_regdata.hpp)

    // device state, all fp64; vectors are [D][N]
    Buf<double> mdata, x, x_new, x_tmp, r, r_new;
    Buf<double> logw, logw_new, wn, work;
    Buf<double> lpri0, llik0, lpri1, llik1, Lg, qv;
    Buf<double> scan_local, ttot, toff, part, scal;
    Buf<double> glk_buf;          // device-side Gaussian L-kernel: mean, both moment sums, parameters (lazy)
    Buf<double> glk_xchg;         // ... over shards: [local row | world gathered rows] of moment sums
    int glk_world = 0;
    // two-phase NUTS launches (smcn_set_nuts_cap): doublings of the first launch, records and list of the parked trees
    int nuts_jcap = 0, nuts_wide2 = 1;
    Buf<double> nuts_resume;
    Buf<unsigned int> nuts_pend;
    Buf<unsigned int> nuts_mq;    // list of the trees parked at the inner level of a launch (smcn_set_nuts_requeue)
    Buf<double> nuts_mq_rec;      // ... and their records ([N][128])
    int nuts_mq_b = 0;                  // ... after this many doublings (0: no inner level)
    bool nuts_mq_used = false;          // the last proposal had an inner level (its hand-over count is checked behind the wait)
    bool nuts_mq_ok = false;            // set by the entry points that wait for the proposal and check that count (smcn_propose_nuts)
    int64_t nuts_parked = 0;            // trees the last launch parked
    Buf<double> stage;  // [N*D] host<->device staging, also [M*D] for target_eval
    Buf<double> stage2;
    Buf<double> cstage;   // SMCN_MODEL_HGLM / ORDINAL / MLGLM: the constrained population the moment kernels read ([ngen][D][N])
    Buf<int32_t> nleap, depth, ndraws, flags;
    Buf<int64_t> idx;
    Buf<unsigned int> queue;
    Buf<double> kin0;     // wave-per-particle NUTS kernels: |r|^2, |r'|^2 and the all-coordinates-moved flag per particle
    Buf<double> kin1;
    Buf<int32_t> moved_i;
    bool kin_valid = false;     // written by the last NUTS launch (consumed by the device-resident re-weighting)
    // Momentum layout.  Targets whose particle fills a wavefront (nuts_wave_kernel: coordinate c on lane c % 64) read and
    // write a particle's momentum as ONE contiguous row: r / r_new then hold [N][D] ("particle-major": 512-byte coalesced
    // rows) instead of the [D][N] every other kernel uses -- converted in place (momentum_dn) before any of those reads them
    bool r_pm = false, r_new_pm = false;
    Buf<unsigned long long> prof;
    Buf<double> tape_d;
    Buf<int64_t> tape_off_d;
    bool momentum_set = false, lg_set = false, q_set = false, u_set = false;
    // device-resident loop (smcn_fast_*)
    Buf<double> hist, ss, lp, gath, hist_x, hist_logw;
    Buf<double> u_res;
    Buf<double> in_rec, out_rec;   // nuts2 per-particle records
    Buf<double> nuts_scratch;                  // HBM tree stacks (large D)
    int64_t fast_K = -1;
    bool fast_hist = false;
    // fused transitions (smcn_super_*)
    int fuse_max = 0;
    int64_t rec_cap = 0;          // transitions the record buffers hold
    int resample_scheme = 0;   // 0 multinomial (reference), 1 systematic
    bool fused_ok = false;     // the model's NUTS kernel takes B > 1 transitions per launch
    bool lane_kernel = false;  // NUTS by nuts3_kernel (one lane per particle)
    int64_t arma_T = 0;        // series length of an arma context
    Buf<double> tb_state, tb_part, tb_local, tb_gath;   // device-side ESS bisection
    int tb_world = 0, tb_blocks = 0;
    int wide_eval = 1;         // nuts3_kernel: lane groups evaluate a wavefront's last stragglers (smcn_set_wide_eval)
    int phase_paths = 1;       // nuts3_kernel: one branch over the bookkeeping no lane needs in an iteration (smcn_set_phase_paths)
    int tree_align = 4;        // nuts3_kernel, a lane per particle: trees start in iterations that are multiples of this (smcn_set_tree_align)
    Buf<unsigned int> wave_iters;   // nuts3_kernel: loop iterations of each wavefront of the last launch (smcn_get_wave_iterations)
    int64_t wave_iters_n = 0;  // ... and how many wavefronts that launch had
    int64_t lane_grid_cap = 0; // nuts3_kernel: wavefronts launched at most (0: one per SIMD; < 0: no cap, a wavefront per 64 particles)
    int lane_segments = 0;     // nuts3_kernel, fewer lanes than particles: segments a block is worked off in (0: auto, 1: whole blocks)
    Buf<unsigned long long> handover;  // [N][segments - 1][VH + 1 pairs] (lane queue: x', running log-weight between segments)
    bool plain_block = false;  // the last smcn_fuse_run ran ONE transition of a model without fused transitions
    // pipelined blocks (smcn_block_*): what follows the NUTS launch (smcn_set_block_post)
    int block_post_mode = 1;   // 1: block_stream_kernel + block_tail_kernel (smcn_block_post.hpp); 0: the separate launches
    bool cnt_zeroed = false;   // smcn_block_launch cleared the block's counters (mode 0 accumulates into them)
    int streamed_g = 0;        // > 0: the post pass of the block was block_stream_kernel on this many cells per generation
    double block_phi = 1.0;    // the block's temperature as smcn_block_launch got it
    // the tail kernel of a one-shard block combines as well, with the arguments smcn_block_stats is expected to bring;
    // smcn_block_stats launches nothing when it brings exactly these (and nobody has rewritten gathB in between)
    struct { int64_t k0 = -1; int B = 0; double n_total = 0.0, phi = 0.0; } tail_combined;
    // ... and leaves the block's last generation in x_next / logw_next as well: smcn_block_commit of the WHOLE block swaps
    // them in instead of copying the generation out of the history -- only while nothing but the block's own entry points
    // (statistics, exchange, wait) has been called since that post pass; anything else falls back to the copies.
    Buf<double> x_next, logw_next;
    uint64_t api_seq = 0;      // entry points called on this context (CHECK_CTX)
    struct { uint64_t seq = 0; int64_t k0 = -1; int B = 0; } next;
    // in-library shard exchange (RCCL) and the routed global resampling (smcn_gres_*)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    Buf<double> g_ttot_all, g_toff_all, g_keys, g_keys_send, g_keys_recv, g_rows_send, g_rows_recv;
    Buf<int32_t> g_dest, g_order;
    int64_t g_serve_cap = 0;
    int g_world = 0;
    smcn_host_target_fn host_fn = nullptr;   // SMCN_MODEL_HOST: the caller's density
    void* host_user = nullptr;
    Buf<double> hc_vec, hc_sc, hc_gp, hc_gl;   // host-target NUTS state
    Buf<int32_t> hc_st;
    std::vector<double> hx, hlp, hll, hgp, hgl;   // host staging of the callback
    Buf<double> n2_ovf;           // v2 kernel: overflow tree-stack levels
    Buf<double> ss_scratch;       // pipelined blocks: step scalars of the inner generations
    DevBuf<double, PinnedMem> rows_h;   // pinned: history rows of the block being validated
    DevBuf<double, PinnedMem> hist_h;   // pinned: the whole scalar history, downloaded behind a run's last block
    bool hist_h_valid = false;
    DevEvent<HipEv, false> ev_rows;     // (no timing: only waited for)
    hipStream_t dl_stream = nullptr;    // history download beside the loop (smcn_history_download)
    Buf<double> dl_stage;
    Buf<double> lpB, gathB, gen_x, gen_logw, cnt, shiftB;

    // NUTS kernel timing (HIP events on the launch stream)
    Event ev0[kTimerRing], ev1[kTimerRing];
    int ev_n = 0;
    double nuts_ms = 0.0;
    int64_t nuts_launches = 0;

    // the post-fit subsystems, none of them touched by the sampler: smcn_loo.hip (pw, ps), smcn_predict.hip (pr, dr; it
    // borrows pw's buffer and events), smcn_summary.hip (sm, cov)
    PwState pw;
    PsState ps;
    PrState pr;
    DrState dr;
    SmState sm;
    CovState cov;
    StState st;      // smcn_api.hip (it runs the models' device functors): the step-size probe
    FcState fc;      // smcn_forecast.hip
    RsState rs;      // smcn_forecast.hip (smcn_residuals.hpp)
};

#define CHECK_CTX(c)            \
    if (!(c)) return -1;         \
    ++(c)->api_seq;              \
    (void)hipSetDevice((c)->device)
#define HIPC(c, call)                                                                         \
    do {                                                                                      \
        const hipError_t e_ = (hipError_t)(call);                                                            \
        if (e_ != hipSuccess) {                                                               \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return -2;                                                                        \
        }                                                                                     \
    } while (0)
#define FAIL(c, msg)      \
    do {                  \
        (c)->err = (msg); \
        return -3;        \
    } while (0)

namespace smcn_host __attribute__((visibility("hidden"))) {
// Waiting for the stream: a blocking hipStreamSynchronize wakes the host ~20-30 us after the last kernel has ended (interrupt,
// scheduler), and a step-by-step iteration waits a dozen times for kernels of a few microseconds.  So: poll the stream for a
// short while first (a query is ~1 us), then block.  SMCN_SPIN_US (default 120) bounds the polling, 0 switches it off.
inline hipError_t stream_wait(hipStream_t s) {
    static const long spin_us = [] { const char* e = getenv("SMCN_SPIN_US"); return e ? atol(e) : 120L; }();
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipErrorNotReady) return q;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= spin_us) break;
        }
    }
    return hipStreamSynchronize(s);
}
inline int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }
// A buffer that may still be in use grows behind a wait for the context's stream.  (Buffers made lazily as a SET are asked
// for by the set's LAST member -- `if (!c->moved_i)` for kin0, kin1, moved_i -- so that a set a failed allocation left
// incomplete is made again; a capacity that is no length -- rec_cap, g_world -- is 0 while its buffers are being made.)
template <class B>
int grow(smcn_ctx* c, B& buf, int64_t need) {
    if (need <= buf.len()) return 0;
    HIPC(c, stream_wait(c->stream));
    HIPC(c, buf.grow(need));
    return 0;
}
inline int ensure_stage(smcn_ctx* c, int64_t n) { return grow(c, c->stage, n); }
inline int ensure_stage2(smcn_ctx* c, int64_t n) { return grow(c, c->stage2, n); }
// The particles a post-fit entry point works on: the caller's x [M][D] uploaded to c->stage, with logw (or zeros) in
// `lw_stage` -- or, x = NULL, the resident ones with their resident log-weights (`who` refuses anything else).
struct Particles {
    const double* xd;
    int64_t rs, cs;
    double* lw;
};
inline int stage_particles(smcn_ctx* c, const char* who, const double* x, const double* logw, int64_t M, double* lw_stage,
                           Particles* P) {
    if (!x) {
        if (M != c->N || logw)
            FAIL(c, std::string(who) + ": the resident particles come with their resident log-weights (x = NULL: logw = NULL, M = N)");
        *P = {c->x, 1, c->N, c->logw};
        return 0;
    }
    const int rc = ensure_stage(c, M * c->D);
    if (rc) return rc;
    HIPC(c, hipMemcpyAsync(c->stage, x, sizeof(double) * M * c->D, hipMemcpyHostToDevice, c->stream));
    if (logw) HIPC(c, hipMemcpyAsync(lw_stage, logw, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    else HIPC(c, hipMemsetAsync(lw_stage, 0, sizeof(double) * M, c->stream));
    *P = {c->stage, c->D, 1, lw_stage};
    return 0;
}

// ---- launchers of kernels another unit owns (all on c->stream; the caller checks hipGetLastError) -----------------------
// smcn_api.hip.  Models whose constrained space is not coordinate-wise have a constrain pass of their own: over M
// particles, particle t's coordinate c at x[(t / Np) * Np * D + (t % Np) * si + c * sc]
bool has_constrain_pass(const smcn_ctx* c);
void launch_constrain_pass(smcn_ctx* c, const double* x, double* out, int64_t M, int64_t Np, int64_t si, int64_t sc);
void launch_constrain_rows(smcn_ctx* c, const double* x, double* out, int64_t M);   // x, out [M][D]: whichever pass the model has
void launch_transpose(smcn_ctx* c, const double* in, double* out, int64_t rows, int64_t cols);
// the blocked inclusive scan of w[M] (scan_tile_kernel) and its nt tile offsets (scan_offsets_kernel)
void launch_scan(smcn_ctx* c, const double* w, int64_t M, int nt, double* local, double* ttot, double* toff);
// smcn_loo.hip.  The header of a call's log-weights, and ll [M][n] of the GLM block L describes (a: pw_args over it)
void launch_pointwise_header(smcn_ctx* c, const double* lw, int64_t M, double* head);
void launch_glm_loglik(smcn_ctx* c, const RegLayout& L, const PwArgs& a, int64_t tiles, int64_t blocks, double* out);
// smcn_predict.hip.  The systematic ancestors of the slots s_first .. s_first + n - 1 of S (smcn_predict_draws' rule) from
// the log-weights lw [M] and their header, the comb's offset uniform on Philox stream `stream`; w, local [M], ttot [nt],
// toff [nt + 1] (nt = the scan tiles of M): work areas
void launch_draw_ancestors(smcn_ctx* c, const double* lw, const double* head, int64_t M, int64_t S, int64_t s_first, int64_t n,
                           uint64_t seed, uint32_t stream, double* w, double* local, double* ttot, double* toff, int64_t* anc);

// ---- the two ends of a draw call (smcn_predict_draws, smcn_forecast_draws) over the work area B (smcn_draw_plan.hpp) ------
// The ancestors of the call's n slots in B + p.o_anc: the caller's, uploaded ahead of ev0, or behind it the systematic
// ones from lw.  check_now: read the weights' finite count and refuse a population without one before the ancestors are
// launched (otherwise draw_finish reads it with the result)
inline int draw_ancestors(smcn_ctx* c, const char* who, Event& ev0, const DrawPlan& p, double* B, const double* lw, int64_t M,
                          int64_t S, int64_t s_first, int64_t n, uint64_t seed, uint32_t stream, const int64_t* ancestors,
                          bool check_now) {
    int64_t* const anc = (int64_t*)(B + p.o_anc);
    if (ancestors) HIPC(c, hipMemcpyAsync(anc, ancestors + s_first, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream));
    HIPC(c, ev0.record(c->stream));
    if (ancestors) return 0;
    launch_pointwise_header(c, lw, M, B);
    if (check_now) {
        double cnt = 1.0;
        HIPC(c, hipMemcpyAsync(&cnt, B + 3, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, stream_wait(c->stream));
        if (cnt == 0.0) FAIL(c, std::string(who) + ": no particle has a finite log-weight");
    }
    launch_draw_ancestors(c, lw, B, M, S, s_first, n, seed, stream, B + p.o_w, B + p.o_loc, B + p.o_tt, B + p.o_to, anc);
    return 0;
}
// Behind the call's last kernel: ev1, the downloads (cnt_d: the finite count to check, or NULL; the ancestors if asked
// for; y [len]), the wait, the kernels' time and the NaN count
inline int draw_finish(smcn_ctx* c, const char* who, Event& ev0, Event& ev1, double* ms, const double* cnt_d, const int64_t* anc,
                       int64_t n, const double* y, int64_t len, double* y_out, int64_t* ancestors_out, int64_t* n_bad_out) {
    HIPC(c, hipGetLastError());
    HIPC(c, ev1.record(c->stream));
    double cnt = 1.0;
    if (cnt_d) HIPC(c, hipMemcpyAsync(&cnt, cnt_d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ancestors_out) HIPC(c, hipMemcpyAsync(ancestors_out, anc, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(y_out, y, sizeof(double) * len, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, stream_wait(c->stream));
    HIPC(c, ev1.since(ev0, ms));
    if (cnt == 0.0) FAIL(c, std::string(who) + ": no particle has a finite log-weight");
    if (n_bad_out) *n_bad_out = count_nan(y_out, len);
    return 0;
}
}  // namespace smcn_host
