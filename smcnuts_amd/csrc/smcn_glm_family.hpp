// The per-observation terms of the regression families, once: every density functor (smcn_models.hpp) and every
// pointwise / predictive walk (smcn_pointwise.hpp, smcn_predict.hpp) calls these.  The family is a wave-uniform runtime
// flag; all of it is inlined.
//   canonical  (glm_canon_obs):  0 bernoulli_logit, 1 poisson_log
//   dispersion (glm_tau_const, glm_disp_obs): 2 normal, y ~ N(eta, sigma^2), sigma = e^tau;
//                                3 neg_binomial_2_log, y ~ NB2(mu = e^eta, phi = e^tau) (Stan's parameterisation)
//   ordinal    (glm_ord_obs): ordered-logistic between two cutpoints
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
