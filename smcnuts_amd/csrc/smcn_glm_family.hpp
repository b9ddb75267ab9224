// The per-observation terms of the regression families, once: every density functor (smcn_models.hpp) and every
// pointwise / predictive walk (smcn_pointwise.hpp, smcn_predict.hpp) calls these.  The family is a wave-uniform runtime
// flag; all of it is inlined.
//   canonical  (glm_canon_obs):  0 bernoulli_logit, 1 poisson_log
//   dispersion (glm_tau_const, glm_disp_obs): 2 normal, y ~ N(eta, sigma^2), sigma = e^tau;
//                                3 neg_binomial_2_log, y ~ NB2(mu = e^eta, phi = e^tau) (Stan's parameterisation)
//   ordinal    (glm_ord_obs): ordered-logistic between two cutpoints
//   tails      (glm_tails): P(Y < y) and P(Y > y) of families 0..3 from the term, for the calibration walk
// NB accuracy where phi >> y + mu: for phi >= kGammaAsym, lgamma(y + phi) - lgamma(phi) - y tau and psi(y + phi) - psi(phi)
// are formed from Stirling's series with log1p(y / phi) -- no lgamma(phi)-sized or phi tau-sized intermediate; below,
// as differences of lgamma / psi, each from a shift up to >= kGammaAsym and the same series (lgamma(phi) and psi(phi)
// are O(1 + |tau|) there; the device library's lgamma inlined into the observation loop made the kernels spill).
// Everything that depends on tau alone is
// formed once per evaluation.  Non-finite: -inf when e^-2tau (normal), e^eta or e^tau (NB) overflows, or e^tau
// leaves the normal range (NB, tau < -708.39).
#pragma once
#include "smcn_device.hpp"

namespace smcn {

constexpr double kLogDblMax = 709.782712893384;        // log(DBL_MAX), rounded down: exp(v) is finite for v <= this
constexpr double kLogDblMinNormal = -708.3964185322641;   // log(DBL_MIN), rounded up

// one observation of a canonical-link family: log-likelihood term and E[y | eta] (the residual is y - mean)
__device__ __forceinline__ void glm_canon_obs(bool poisson, double eta, double y, double lgy, double& term, double& mean) {
    if (poisson) {
        const double mu = exp_fast(eta);
        term = ((y == 0.0 ? 0.0 : y * eta) - mu) - lgy;
        term = mu < kInf ? term : -kInf;             // poisson_log_lpmf: exp(eta) overflows
        mean = mu;
    } else {
        // y eta - softplus(eta), softplus(eta) = max(eta, 0) + log1p(e^-|eta|); y eta - max(eta, 0) is min(eta, 0) for
        // y = 1 and -max(eta, 0) for y = 0, without the cancellation
        const double t = exp_fast(-fabs(eta));
        double inv;
        const double l1 = log1p_pos(t, inv);          // inv = 1 / (1 + e^-|eta|) = sigmoid(|eta|)
        term = (y != 0.0 ? fmin(eta, 0.0) : -fmax(eta, 0.0)) - l1;
        mean = eta >= 0.0 ? inv : t * inv;
    }
}

// what one evaluation derives from tau alone (the two dispersion families share the registers)
struct TauConst {
    double tau;
    double phi, iphi;             // normal: e^-2tau, -tau - log(2 pi) / 2;  NB: e^tau, 1 / phi
    double c1, c2;                // NB: Stirling and digamma tails of phi (big), or lgamma(phi) and psi(phi)
    bool big, bad;
};

__device__ __forceinline__ TauConst glm_tau_const(bool nb, double tau) {
    TauConst k;
    k.tau = tau;
    if (!nb) {
        k.bad = -2.0 * tau > kLogDblMax;
        k.phi = exp_fast(-2.0 * tau);
        k.iphi = -tau - 0.5 * kLog2Pi;
        k.c1 = k.c2 = 0.0;
        k.big = false;
    } else {
        k.bad = !(tau <= kLogDblMax && tau >= kLogDblMinNormal);
        k.phi = k.bad ? 1.0 : exp_fast(tau);
        k.iphi = 1.0 / k.phi;
        k.big = k.phi >= kGammaAsym;
        if (k.big) {
            k.c1 = stirling_tail(k.iphi);
            k.c2 = digamma_tail(k.iphi);
        } else {
            lgamma_digamma_pos(k.phi, k.c1, k.c2);
        }
    }
    return k;
}

// one observation of a dispersion family: log-likelihood term, d term / d eta and d term / d tau
__device__ __forceinline__ void glm_disp_obs(bool nb, const TauConst& k, double eta, double y, double lgy, double& term,
                                             double& d, double& gt) {
    if (!nb) {
        const double r = y - eta;
        const double rw = r * k.phi;                 // (phi: e^-2tau, iphi: -tau - log(2 pi) / 2)
        const double q = r * rw;
        term = fma(-0.5, q, k.iphi);
        d = rw;
        gt = q - 1.0;
    } else {
        const double x = y + k.phi;
        // A = lgamma(y + phi) - lgamma(phi) [- y tau when big], B = psi(y + phi) - psi(phi); both 0 at y = 0.  One
        // pair of asymptotic tails either way: at y + phi (big), or at y + phi shifted up to >= kGammaAsym
        double P, S;
        const double xs = k.big ? x : gamma_shift(y == 0.0 ? kGammaAsym : x, P, S);
        const double ix = 1.0 / xs;
        const double st = stirling_tail(ix), dt = digamma_tail(ix);
        double A, B, ts;
        if (k.big) {
            double ir;                                   // 1 / (1 + y / phi) = phi / x
            const double l1 = log1p_pos(y * k.iphi, ir);   // log(x / phi)
            A = fma(x - 0.5, l1, -y) + (st - k.c1);
            B = fma(0.5 * y, ix * k.iphi, l1) - (dt - k.c2);
            ts = 0.0;
        } else {                                         // (xs >= 10 and P >= 1: log_ge1)
            const double lx = log_ge1(xs);
            A = ((fma(xs - 0.5, lx, -xs) + (0.5 * kLog2Pi + st)) - log_ge1(P)) - k.c1;
            B = (((lx - 0.5 * ix) - dt) - S) - k.c2;
            ts = k.tau;
        }
        A = y == 0.0 ? 0.0 : A;
        B = y == 0.0 ? 0.0 : B;
        // softplus(eta - tau) = log(mu + phi) - tau, sigmoid(eta - tau) = mu / (mu + phi) and its complement
        const double z = eta - k.tau;
        const double t = exp_fast(-fabs(z));
        double inv;
        const double sp = fmax(z, 0.0) + log1p_pos(t, inv);
        const double ti = t * inv;
        const double sg = z >= 0.0 ? inv : ti, sc = z >= 0.0 ? ti : inv;
        term = ((A - lgy) - x * sp) + y * (eta - ts);
        term = eta <= kLogDblMax ? term : -kInf;           // e^eta overflows
        d = fma(-x, sg, y);
        gt = fma(k.phi, (B - sp) + sg, -y * sc);
    }
}

// ---- the predictive tails at an observation (smcn_calibration.hpp): lo = P(Y < y), up = P(Y > y) -------------------------
// Each tail keeps RELATIVE accuracy: the smaller one comes from a convergent series or continued fraction of non-negative
// size whose prefactor is pmf = exp(term) times an O(1) factor -- the term the walk has formed, with its Stirling-based
// lgamma differences, never a fresh exp(a log x - x - lgamma(a)) -- and the larger one is the complement 1 - pmf - other.
// Every loop runs at most kCalMaxIter iterations; a tail that has not converged by then is reported (false), never
// returned as if it had.  The bodies hold multiplications, reciprocals (rcp_nr) and compares only: nothing that spills.
constexpr int kCalMaxIter = 2048;

// poisson_log.  The series that runs AWAY from the mode, so that its terms fall from the first one on:
//   y + 1 > mu:  up = pmf sum_{k >= 1} mu^k / ((y + 1) .. (y + k))          (P(y + 1, mu))
//   otherwise:   lo = pmf sum_{k = 1..y} y (y - 1) .. (y - k + 1) / mu^k    (Q(y, mu); the sum ends by itself at k = y)
// stopped at the first term below 1e-17 of the sum.  About 8.2 sqrt(mu) terms at the mode, 39 / log(1 / ratio) away from it.
__device__ __forceinline__ bool glm_poisson_tails(double y, double mu, double pmf, double& lo, double& up) {
    const bool upper = y + 1.0 > mu;
    const double imu = rcp_nr(mu);                   // (upper, or mu >= 1)
    double t = 1.0, s = 0.0;
    bool conv = false;
#pragma unroll 1
    for (int k = 1; k <= kCalMaxIter; ++k) {
        const double kd = (double)k;
        t *= upper ? mu * rcp_nr(y + kd) : (y - (kd - 1.0)) * imu;
        s += t;
        if (t <= 1e-17 * s) {                        // (t = 0: the lower sum has ended, or mu = 0)
            conv = true;
            break;
        }
    }
    const double tail = pmf * s, rest = fmax((1.0 - pmf) - tail, 0.0);
    lo = y == 0.0 ? 0.0 : (upper ? rest : tail);
    up = upper ? tail : rest;
    return conv;
}

// The continued fraction of the regularised incomplete beta function without its prefactor,
// I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) h, by the modified Lentz recurrence, two partial numerators per iteration; it
// converges in O(sqrt(max(a, b))) iterations for x < (a + 1) / (a + b + 2).  Stopped when a step changes h by <= 2 ulp.
__device__ __forceinline__ bool glm_beta_cf(double a, double b, double x, double& h) {
    constexpr double tiny = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x * rcp_nr(qap);
    d = fabs(d) < tiny ? tiny : d;
    d = rcp_nr(d);
    h = d;
    bool conv = false;
#pragma unroll 1
    for (int m = 1; m <= kCalMaxIter; ++m) {
        const double md = (double)m, m2 = md + md, am2 = a + m2;
        const double i1 = rcp_nr((qam + m2) * am2), i2 = rcp_nr(am2 * (qap + m2));
        double aa = md * (b - md) * x * i1;
        d = fma(aa, d, 1.0);
        d = fabs(d) < tiny ? tiny : d;
        c = fma(aa, rcp_nr(c), 1.0);
        c = fabs(c) < tiny ? tiny : c;
        d = rcp_nr(d);
        h *= d * c;
        aa = -(a + md) * (qab + md) * x * i2;
        d = fma(aa, d, 1.0);
        d = fabs(d) < tiny ? tiny : d;
        c = fma(aa, rcp_nr(c), 1.0);
        c = fabs(c) < tiny ? tiny : c;
        d = rcp_nr(d);
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= 4.5e-16) {
            conv = true;
            break;
        }
    }
    return conv;
}

// neg_binomial_2_log with q = mu / (mu + phi), pr = 1 - q (both from sigmoid(+-(eta - tau)), neither as 1 - the other):
//   q (y + phi + 3) < y + 2:  up = I_q(y + 1, phi) = pmf q (y + phi) / (y + 1) h(y + 1, phi, q)
//   otherwise:                lo = I_pr(phi, y)    = pmf y / phi h(phi, y, pr)
// One of the two conditions of glm_beta_cf always holds; the first is taken where both do.
__device__ __forceinline__ bool glm_nb_tails(double y, double phi, double iphi, double z, double pmf, double& lo, double& up) {
    const double t = exp_fast(fmax(-fabs(z), -800.0));
    const double inv = rcp_nr(1.0 + t), ti = t * inv;
    const double q = z >= 0.0 ? inv : ti, pr = z >= 0.0 ? ti : inv;
    const bool upper = q * (y + phi + 3.0) < y + 2.0;
    double h;
    const bool conv = glm_beta_cf(upper ? y + 1.0 : phi, upper ? phi : y, upper ? q : pr, h);
    const double pre = upper ? q * (y + phi) * rcp_nr(y + 1.0) : y * iphi;
    const double tail = pmf * pre * h, rest = fmax((1.0 - pmf) - tail, 0.0);
    lo = y == 0.0 ? 0.0 : (upper ? rest : tail);
    up = upper ? tail : rest;
    return conv;
}

// lo and up of family `fam` at (eta, y) from the finite term the walk formed (k: the dispersion families' constants);
// false: a tail reached the iteration bound
__device__ __forceinline__ bool glm_tails(int fam, double eta, double y, double term, const TauConst& k, double& lo, double& up) {
    if (fam == 0) {
        const double t = exp_fast(fmax(-fabs(eta), -800.0));
        const double inv = rcp_nr(1.0 + t), ti = t * inv;
        // y = 1: lo = sigmoid(-eta); y = 0: up = sigmoid(eta)
        lo = y != 0.0 ? (eta >= 0.0 ? ti : inv) : 0.0;
        up = y != 0.0 ? 0.0 : (eta >= 0.0 ? inv : ti);
        return true;
    }
    if (fam == 2) {
        const double z = (y - eta) * exp_fast(-k.tau) * 0.70710678118654752440;
        lo = 0.5 * erfc(-z);
        up = 0.5 * erfc(z);
        return true;
    }
    const double pmf = exp_fast(fmax(term, -800.0));
    if (fam == 1) return glm_poisson_tails(y, exp_fast(eta), pmf, lo, up);
    return glm_nb_tails(y, k.phi, k.iphi, eta - k.tau, pmf, lo, up);
}

// one ordinal observation with label y of K = Km1 + 1 classes, lo = c_y (y >= 1) and hi = c_{y+1} (y <= K - 2):
// log-likelihood term, d / d eta, and the partials of the lower and the upper cutpoint
__device__ __forceinline__ void glm_ord_obs(int Km1, double eta, int y, double lo, double hi, double& term, double& de,
                                            double& glo, double& ghi) {
    const bool hl = y >= 1, hh = y < Km1;
    const double a1 = lo - eta, a2 = eta - hi;
    // (exp_fast flushes below -800; a NaN stays NaN)
    auto ex = [](double a) { return exp_fast(a < -800.0 ? -800.0 : a); };
    const double t1 = ex(-fabs(a1)), t2 = ex(-fabs(a2));
    double i1, i2;
    const double sp1 = fmax(a1, 0.0) + log1p_pos(t1, i1);   // softplus(a1); i1 = sigmoid(|a1|)
    const double sp2 = fmax(a2, 0.0) + log1p_pos(t2, i2);
    const double s1 = a1 >= 0.0 ? i1 : t1 * i1, s2 = a2 >= 0.0 ? i2 : t2 * i2;
    term = -((hl ? sp1 : 0.0) + (hh ? sp2 : 0.0));
    term = finite_d(eta) ? term : -kInf;
    glo = hl ? -s1 : 0.0;
    ghi = hh ? s2 : 0.0;
    de = -(glo + ghi);
}

}  // namespace smcn
