"""The references of tests/_weights.py against independent code, so that a wrong reference cannot bless a wrong kernel:
the Metropolis decisions against smcnuts_amd.proposal.utils.hmc_accept_mask, the ESS function against the host _ess of
ESSTempering.calculate_phi, the project's bisect against scipy.optimize.bisect, the class rules on a hand-written table, the
margin builder's refusal of a u on the threshold, and a float64 stand-in for the device (sums in another order) on every
tempering case of tests/test_gpu_weights.py."""
import math

import numpy as np
import pytest

import _weights as W

INF, NAN = math.inf, math.nan


# ---- the Metropolis decisions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("D,N", [(1, 2), (4, 257), (64, 64)])
def test_decisions_equal_hmc_accept_mask(D, N, phi):
    from smcnuts_amd.proposal.utils import hmc_accept_mask
    tl, tk, x, x_new, r, r_new, u, near = W.accept_inputs(D, N, phi, 300 + N)
    parts = (tl[:N], tk[:N], tl[N:], tk[N:])
    W.set_near(W.decisions_ref(*parts, r, r_new, x_new, phi, u), u, near)
    dec = W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, phi, u))
    keep = hmc_accept_mask(W.combine64(tl[:N], tk[:N], phi), W.combine64(tl[N:], tk[N:], phi), r, r_new, x_new, u)
    np.testing.assert_array_equal(dec.accept, keep)
    if N >= 32:
        # the edge rows decide as the reference's Python does: u = 0 against an underflowed prob accepts, the smallest positive u
        # does not; a NaN ratio accepts; an infinite coordinate rejects whatever u is, a NaN coordinate does not
        assert dec.accept[1] and not dec.accept[2] and dec.accept[6] and dec.dH_cls[6] == W.NAN
        assert D == 1 or (not dec.accept[7] and not dec.accept[8] and dec.accept[9])
        assert [bool(dec.accept[i]) for i in near] == [True, False, True, False]
    # the share of rows left out of a decision comparison is zero by construction
    assert np.all(dec.margin >= 100.0 * dec.bound)
    # the float64 probability is within the stated bound of the exact one
    with np.errstate(all="ignore"):
        k0, k1 = np.einsum("ij,ij->i", r, r), np.einsum("ij,ij->i", r_new, r_new)
        dH = (W.combine64(tl[N:], tk[N:], phi) - 0.5 * k1) - (W.combine64(tl[:N], tk[:N], phi) - 0.5 * k0)
        p64 = np.minimum(1.0, np.exp(dH))
    ok = np.isfinite(dH) & (dH > -700)
    pe = np.array([float(p) for p in dec.prob])
    assert np.all(np.abs(p64[ok] - pe[ok]) <= dec.bound[ok] * pe[ok] + 1e-300)


def test_margin_builder_refuses_a_uniform_on_the_threshold():
    tl, tk, x, x_new, r, r_new, u, near = W.accept_inputs(4, 64, 1.0, 1)
    parts = (tl[:64], tk[:64], tl[64:], tk[64:])
    dec = W.decisions_ref(*parts, r, r_new, x_new, 1.0, u)
    W.set_near(dec, u, near)
    W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, 1.0, u))          # 1e-9 off: accepted by the builder
    for scale in (1.0, 1.0 + 1e-13, 1.0 - 1e-13):
        u[near[0]] = float(dec.prob[near[0]]) * scale
        with pytest.raises(ValueError, match="on the threshold"):
            W.require_margins(W.decisions_ref(*parts, r, r_new, x_new, 1.0, u))


# ---- the class rules --------------------------------------------------------------------------------------------------------
def test_class_rules_on_a_hand_written_table():
    #                 lpri  llik   phi   combine
    table = [(-1.0, -2.0, 0.5, -2.0),
             (-1.0, -INF, 0.0, -INF),        # 0 * -inf is NaN, and NaN is not finite
             (-1.0, -INF, 0.5, -INF),
             (-INF, -INF, 0.0, -INF),
             (-INF, -INF, 1.0, -INF),
             (-1.0, INF, 1.0, -INF),         # +inf is not finite either: a failed density
             (INF, -1.0, 0.0, -INF),
             (INF, -INF, 1.0, -INF),
             (NAN, -1.0, 1.0, -INF),
             (1e308, 1e308, 1.0, -INF),      # overflow
             (1e300, -1e300, 1.0, 0.0)]
    for lpri, llik, phi, want in table:
        got = W.combine64(np.array([lpri]), np.array([llik]), phi)[0]
        assert got == want, (lpri, llik, phi, got)
        mp = W.combine_mp([lpri], [llik], phi)[0]
        assert (mp is None) == (want == -INF) and (mp is None or float(mp) == want)
    # differences: classes by IEEE, left to right
    lw = np.array([0.5, 0.5, -INF, NAN, 0.5, 0.5])
    lp = np.array([-1.0, -1.0, -1.0, -1.0, -INF, 1e300])
    lk = np.array([-2.0, -INF, -2.0, -2.0, -1.0, -1e300])
    ref = W.tempered_difference_ref(lw, lp, lk, 1.0, 0.0)
    # row 1: -inf - (-inf) (phi = 0 gives 0 * -inf = NaN -> -inf): NaN;  row 4: both -inf: NaN;  row 5: 0 - 1e300
    np.testing.assert_array_equal(ref.cls, [W.FINITE, W.NAN, W.NINF, W.NAN, W.NAN, W.FINITE])
    assert ref.hi[0] == 0.5 - 2.0 and ref.hi[5] == 0.5 - 1e300
    same = W.tempered_difference_ref(None, lp, lk, 0.3, 0.3)
    np.testing.assert_array_equal(same.cls, [W.FINITE, W.NAN, W.FINITE, W.FINITE, W.NAN, W.FINITE])
    assert np.all(same.hi[same.cls == W.FINITE] == 0.0)
    # re-weighting: p_x = -inf gives +inf, p_xn = -inf gives -inf, both NaN
    z = np.zeros((4, 2))
    rw = W.reweight_ref(np.zeros(4), np.array([-1.0, -INF, -1.0, -INF]), np.full(4, -1.0),
                        np.array([-1.0, -1.0, -INF, -INF]), np.full(4, -1.0), z, z)
    np.testing.assert_array_equal(rw.cls, [W.FINITE, W.PINF, W.NINF, W.NAN])
    assert rw.hi[0] == 0.0
    # initial weights
    iw = W.init_weights_ref(np.array([-1.0, -INF]), np.array([-2.0, -1.0]), 0.5, logq0=np.array([-3.0, -3.0]))
    np.testing.assert_array_equal(iw.cls, [W.FINITE, W.NINF])
    assert iw.hi[0] == 1.0


def test_values_are_exact_where_float64_is():
    """Small dyadic inputs: every float64 operation is exact, so the 40-digit value equals the float64 one."""
    rng = np.random.default_rng(3)
    q = lambda a: np.round(a * 256.0) / 256.0
    n, D = 50, 4
    lw, a, b, c, d = (q(rng.standard_normal(n) * 4) for _ in range(5))
    r, rn = q(rng.standard_normal((n, D))), q(rng.standard_normal((n, D)))
    L, qq = q(rng.standard_normal(n)), q(rng.standard_normal(n))
    ref = W.reweight_ref(lw, a, b, c, d, r, rn, L=L, q=qq)
    np.testing.assert_array_equal(ref.hi, lw + (c + d) - (a + b) + L - qq)
    assert np.all(ref.lo == 0.0)
    ref = W.reweight_ref(lw, a, b, c, d, r, rn)
    want = lw + (c + d) - (a + b) - 0.5 * np.sum(rn * rn, axis=1) + 0.5 * np.sum(r * r, axis=1)
    assert np.all(np.abs(ref.hi - want) <= ref.bound) and np.all(ref.bound < 1e-13)
    T = W.Tempered(a, b, 0.0)
    assert T.exactly_computable(0.5) and not W.Tempered(a, b, 0.3).exactly_computable(0.5)
    p = T.partials(0.5)
    assert p["mx64"] == np.max(0.5 * b) and p["cnt"] == int(np.sum(0.5 * b == np.max(0.5 * b)))


# ---- the ESS function -------------------------------------------------------------------------------------------------------
class _PartsTarget:
    def __init__(self, lpri, llik):
        self.parts = (lpri, llik)

    def logpdf_parts(self, x):
        return self.parts


@pytest.mark.parametrize("N", [2, 64, 1000, 4097, 20001])
def test_ess_function_equals_the_host_ess(N, monkeypatch):
    """ESSTempering.calculate_phi's own _ess (the host path of the project, plain NumPy) against f_exact, and the phi it
    returns against the root property."""
    from smcnuts_amd.tempering import adaptive_tempering as at
    for kind in ("distinct", "repeated"):
        lpri, llik = W.population(kind, N, seed=1)
        for po in W.PHI_OLD:
            T = W.Tempered(lpri, llik, po)
            grabbed = []
            monkeypatch.setattr(at, "bisect", lambda f, a, b: grabbed.append(f) or a)
            tempering = at.ESSTempering(N, _PartsTarget(lpri, llik), alpha=0.5)
            p_old = W.combine64(lpri, llik, po)
            tempering.calculate_phi([None, p_old, po])
            monkeypatch.undo()
            if not grabbed:                       # ESS(1) >= N / 2: no bisection
                assert T.f(0.5 * N)(1.0) >= 0
                continue
            f64, f = grabbed[0], T.f(0.5 * N)
            for phi in (po, po + 1e-3, 0.5, 0.9, 1.0):
                b = T.ess_bound(T.partials(phi, strict=False))
                assert abs(f64(phi) - f(phi)) <= b, (kind, N, po, phi, f64(phi), f(phi), b)
            phi = at.ESSTempering(N, _PartsTarget(lpri, llik), alpha=0.5).calculate_phi([None, p_old, po])
            if W.has_root(T, 0.5 * N):
                W.check_root(T, phi, 0.5 * N, f"host calculate_phi {kind} N={N} phi_old={po}")


# ---- bisect against scipy ---------------------------------------------------------------------------------------------------
def test_bisect_equals_scipy():
    from scipy.optimize import bisect as sp_bisect
    from smcnuts_amd.tempering.adaptive_tempering import bisect
    cases = [(lambda x: 0.3 - x, 0.0, 1.0), (lambda x: math.exp(-5 * x) - 0.2, 0.0, 1.0), (lambda x: x * x - 0.5, 0.0, 1.0),
             (lambda x: 0.5 - x, 0.5, 1.0),                              # f(a) == 0: the left end
             (lambda x: x - 1.0, 0.0, 1.0),                              # f(b) == 0
             (lambda x: math.cos(40 * x), 1e-4, 1.0), (lambda x: 1e-300 * (0.7 - x), 0.3, 1.0),
             (lambda x: (1 - 5e-10) - x, 1 - 1e-9, 1.0)]                 # a bracket narrower than 1000 xtol
    for f, a, b in cases:
        assert bisect(f, a, b) == sp_bisect(f, a, b), (a, b)
    for f, a, b, exc in [(lambda x: x + 1.0, 0.0, 1.0, ValueError), (lambda x: -x - 1.0, 0.0, 1.0, ValueError),
                         (lambda x: NAN, 0.0, 1.0, ValueError)]:
        with pytest.raises(exc):
            bisect(f, a, b)
        with pytest.raises(exc):
            sp_bisect(f, a, b)
    with pytest.raises(RuntimeError):
        bisect(lambda x: 0.3 - x, 0.0, 1.0, maxiter=5)
    with pytest.raises(RuntimeError):
        sp_bisect(lambda x: 0.3 - x, 0.0, 1.0, maxiter=5)


# ---- a float64 stand-in for the device on every tempering case of the GPU file ------------------------------------------------
def _standin_bisect(lpri, llik, po, target):
    from smcnuts_amd.parallel import combine_lse_partials
    from smcnuts_amd.tempering.adaptive_tempering import bisect

    def f(phi):
        _, sw = combine_lse_partials(W.standin_partials(lpri, llik, po, phi)[None, :])
        with np.errstate(all="ignore"):
            return 1.0 / sw - target
    if f(1.0) >= 0:
        return 1.0, 0
    try:
        return bisect(f, po, 1.0), 0
    except ValueError:
        return NAN, 2
    except RuntimeError:
        return NAN, 3


@pytest.mark.parametrize("N", W.TEMPER_N)
@pytest.mark.parametrize("kind", W.TEMPER_KINDS + ("masked",))
def test_a_float64_stand_in_passes_the_tempering_cases(kind, N):
    """The checks of test_gpu_weights.test_temper_partials / test_temper_bisect with a NumPy stand-in in the device's place:
    they hold for a correct float64 evaluation whose sums run in another order, with room to spare."""
    if kind == "masked" and N == 1:
        kind = "distinct"
    lpri, llik = W.population(kind, N)
    worst = 0.0
    for po in W.PHI_OLD:
        T = W.Tempered(lpri, llik, po)
        for pn in (0.25, 0.5, 1.0):
            dev = W.standin_partials(lpri, llik, po, pn)
            if np.any(T.rows_cls(pn) == W.NAN):
                assert np.isnan(dev[0])
                continue
            p = T.partials(pn)
            assert dev[1] == p["cnt"]
            assert abs(dev[0] - p["mx64"]) <= p["bv"] + W.U * abs(p["mx64"])
            if T.exactly_computable(pn):
                assert dev[0] == p["mx64"]
            e1, e2 = T.sum_bounds(p)
            assert abs(dev[2] - p["s1"]) <= e1 * p["s1"] + W.U * p["s1"] and abs(dev[3] - p["s2"]) <= e2 * p["s2"] + W.U * p["s2"]
        for alpha in (0.5, 0.9):
            phi, st = _standin_bisect(lpri, llik, po, alpha * N)
            W.check_outcome(T, alpha * N, phi, st, f"stand-in {kind} N={N} phi_old={po} target={alpha} N")
    worst = W.SHARES.get("bisect root", (0.0, 0.0))[1]
    print(f"stand-in {kind} N={N}: largest share of the half-width used so far {worst:.2f}")


def test_the_stand_in_in_a_narrow_bracket():
    N, po = 1000, 1.0 - 1e-9
    lpri, llik = W.population("steep", N)
    T = W.Tempered(lpri, llik, po)
    for alpha in (0.5, 0.9):
        assert W.has_root(T, alpha * N)
        phi, st = _standin_bisect(lpri, llik, po, alpha * N)
        assert po < phi < 1.0
        W.check_outcome(T, alpha * N, phi, st, f"stand-in steep target={alpha} N")
