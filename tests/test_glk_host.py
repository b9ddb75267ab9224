"""The reference, the yardsticks and the case list of the Gaussian L-kernel tests (tests/_glk.py), on the CPU: what
tests/test_gpu_glk.py measures the device against must itself be right, and the populations must sit where the device's
decision is forced -- comfortably inside, beyond, and next to kGlkMaxCond -- before a device is asked.

Every particle of every case enters every comparison: nothing is masked or dropped."""
import numpy as np
import pytest

import _glk as G

from oracle import oracle as orc

U = G.U64
NAMES = list(G.CASES)


def _cls(name):
    return G.decision(G.exact_case(name), G.CASES[name]["D"])


def _well_conditioned(name):
    """Both condition numbers small, the mean not far, and more than 2 D + 1 distinct particles: with fewer the Schur
    complement c_rr - B c_xr cancels to (nearly) nothing and float64 loses |c_rr| / lambda_min(cov) on top of cond u."""
    ex, c = G.exact_case(name), G.CASES[name]
    determined = (c.get("uniq") or c["N"]) - 1 > 2 * c["D"]
    return not ex["singular"] and max(ex["cond_xx"], ex["cond_cov"]) < 1e4 and "far" not in c and determined


def test_populations_are_fixed_and_shaped():
    for name, c in G.CASES.items():
        r, x = G.population(name)
        assert r.shape == x.shape == (c["N"], c["D"]) and np.all(np.isfinite(r)) and np.all(np.isfinite(x))
        assert G.population(name)[1] is x and not x.flags.writeable          # computed once, shared, left unchanged
        if "uniq" in c:
            assert np.unique(np.hstack([r, x]), axis=0).shape[0] == c["uniq"]
    assert abs(G.population("d8_far")[1].mean()) > 9e5 and G.population("d8_far")[1].std(axis=0).max() < 10


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ("d5_d", "d13_u13")])
def test_exact_against_the_float64_formulations(name):
    """exact() against the oracle's restatement and GaussianApproxLKernel.calculate_L where float64 is comfortable: a
    backward-stable float64 route through two D x D inverses is within ~ D cond u of the exact value relative to
    |c0| + maha / 2 (bound used: 64 D (cond(c_xx) + cond(cov)) u); a wrong formula in exact() misses by O(1)."""
    if not _well_conditioned(name):
        assert not G.exact_case(name)["singular"]           # (the ill-conditioned cases: test_yardsticks_stay_finite)
        return
    r, x = G.population(name)
    ex = G.exact_case(name)
    D = G.CASES[name]["D"]
    bound = 64 * D * (ex["cond_xx"] + ex["cond_cov"]) * U
    for what, L in (("oracle", orc.gaussian_lkernel(r, x)), ("calculate_L", G.host_L(r, x)), ("cholesky", G.chol_L(r, x))):
        err = G.rel_err(L, ex)
        print(f"{name} {what}: {err / U:.3g} u, bound {bound / U:.3g} u")
        assert err <= bound, (name, what, err, bound)
    # the parts test_gpu_glk.py hands to glk_logpdf_kernel give the same values through the plain formula
    L = G.logpdf_np(r, x, ex["mu_x"], ex["m0"], ex["B"], ex["U"], ex["c0"])
    assert G.rel_err(L, ex) <= bound
    np.testing.assert_allclose(ex["scale"], abs(ex["c0"]) + 0.5 * ex["maha"], rtol=1e-15)
    np.testing.assert_allclose(ex["L"], ex["c0"] - 0.5 * ex["maha"], rtol=1e-14, atol=1e-14 * abs(ex["c0"]))


def test_exact_sees_a_singular_covariance():
    for name in ("d5_d", "d13_u13"):            # N - 1 < D, and fewer than D + 1 distinct particles
        ex = G.exact_case(name)
        assert ex["singular"] and ex["cond_xx"] == np.inf
    ex = G.exact_case("d5_d1")                  # N - 1 = D: c_xx barely regular, r an exact linear function of x:
    assert not ex["singular"] and abs(ex["cond_cov"] - 1.0) < 1e-6      # the Schur complement is 0 and cov the ridge alone


@pytest.mark.parametrize("D", [1, 2, 5, 13, 32])
def test_estimate_brackets_the_condition_number(D):
    """The algebra of the device's estimate (smcn_glk.hpp), in NumPy: cond_2 <= trace(M) |M^-1|_F <= D^1.5 cond_2 for
    symmetric positive definite M -- trace >= lambda_max and <= D lambda_max; |M^-1|_F >= 1 / lambda_min and
    <= sqrt(D) / lambda_min.  Both ends are attained (rank-one dominated; the identity), so neither can be tightened."""
    rng = np.random.default_rng(D)
    for k in range(20):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        lam = 10.0 ** rng.uniform(-3 * (k % 3), 0.0, D)
        M = (Q * lam) @ Q.T
        M = 0.5 * (M + M.T)
        ev = np.linalg.eigvalsh(M)
        cond = ev[-1] / ev[0]
        est = np.trace(M) * np.linalg.norm(np.linalg.inv(M), "fro")
        assert cond * (1 - 1e-9) <= est <= D ** 1.5 * cond * (1 + 1e-9)
    est_eye = np.trace(np.eye(D)) * np.linalg.norm(np.eye(D), "fro")
    assert est_eye == pytest.approx(D ** 1.5)


def test_case_list_holds_all_three_classes():
    """The conditions on the case list, from the exact condition numbers (eigenvalues at 50 digits): must accept --
    1.01 D^1.5 cond < 1e8 for both matrices, the device's estimate cannot reach kGlkMaxCond; must refuse -- cond > 1.01e8
    for either or c_xx singular, the estimate cannot stay below; either -- the rest."""
    cls = {n: _cls(n) for n in NAMES}
    for n in NAMES:
        ex = G.exact_case(n)
        print(f"{n:9s} cond(c_xx) {ex['cond_xx']:.3g} cond(cov) {ex['cond_cov']:.3g} -> {cls[n]}")
    count = lambda c: sum(v == c for v in cls.values())
    assert count("accept") >= 10 and count("refuse") >= 3 and count("either") >= 1, cls
    for n, want in G.INTENDED.items():
        assert cls[n] == want, (n, cls[n], want)
    # the regimes the table names are where they should be
    assert G.exact_case("d5_d3")["cond_cov"] > 1e6 and G.exact_case("d13_u20")["cond_cov"] > 1e6     # ridge-held
    assert cls["d5_d3"] == cls["d5_d1"] == cls["d13_u20"] == cls["d32_65"] == cls["d8_far"] == "accept"


@pytest.mark.parametrize("name", NAMES)
def test_yardsticks_stay_finite(name):
    """Wherever the device must answer, both float64 restatements answer too, with finite values: the tolerance of
    test_gpu_glk.py (MARGIN x the larger of their errors) exists on every accepted case.  Where the device must refuse
    the reference's own calls answer with finite values, the case is listed in HOST_ANSWERS (test_gpu_glk.py then follows
    GaussianApproxLKernel.apply onto its host path)."""
    r, x = G.population(name)
    ex = G.exact_case(name)
    if _cls(name) == "refuse":
        assert (name in G.HOST_ANSWERS) == bool(np.all(np.isfinite(G.host_L(r, x))))
        return
    eh, ec = G.rel_err(G.host_L(r, x), ex), G.rel_err(G.chol_L(r, x), ex)
    print(f"{name}: calculate_L {eh / U:.3g} u, cholesky {ec / U:.3g} u")
    assert np.isfinite(eh) and np.isfinite(ec)
    assert G.yardstick(r, x, ex) == max(eh, ec, 16 * U)


@pytest.mark.parametrize("D,N", [(1, 1), (3, 7), (5, 65), (17, 129), (64, 3)])
@pytest.mark.parametrize("centred", [False, True])
def test_exact_sums(D, N, centred):
    """exact_sums against a float64 restatement (np.sum of the same terms) within N u of the magnitudes, the mpmath and
    the long-double route against each other, and the layout of smcn_gauss_lkernel_sums (_unpack_sums reads it)."""
    from smcnuts_amd.lkernel.gaussian_lkernel import _unpack_sums
    rng = np.random.default_rng(100 * D + N)
    r, x = rng.standard_normal((N, D)) * 3.0, rng.standard_normal((N, D)) + 2.0
    X = np.hstack([-r, x])
    shift = X.mean(axis=0) if centred else np.zeros(2 * D)
    s, m = G.exact_sums(r, x, shift)
    v, M2 = _unpack_sums(s, 2 * D)
    Xc = X - shift
    assert np.all(np.abs(v - Xc.sum(axis=0)) <= (N + 2) * U * np.abs(Xc).sum(axis=0))
    assert np.all(np.abs(M2 - Xc.T @ Xc) <= (N + 4) * U * (np.abs(Xc).T @ np.abs(Xc)))
    assert np.all(m >= np.abs(s))
    keep = G.MP_WORK
    try:
        G.MP_WORK = 0                              # the long-double route on the same input
        s2, m2 = G.exact_sums(r, x, shift)
    finally:
        G.MP_WORK = keep
    assert np.all(np.abs(s2 - s) <= 4 * U * m)
    np.testing.assert_allclose(m2, m, rtol=4 * U)


def test_sums_depth_follows_the_launch():
    assert G.sums_depth(1, 1) == 4 + 6 + 1 + 1 + 8
    assert G.sums_depth(1000, 17) == 1 + 6 + 1 + 1 + 8                      # 16 tiles of 64, 16 blocks
    assert G.sums_depth(64 * 1024 + 65, 17) == 1 + 6 + 2 + 4 + 8            # 1026 tiles on 1024 blocks: the grid-stride loop
    assert G.sums_depth(256 * 1024 + 257, 2) == 4 + 6 + 2 + 4 + 8
