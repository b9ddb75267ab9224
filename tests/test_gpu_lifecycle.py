"""A context's owned device buffers (smcnuts_amd/csrc/smcn_devbuf.hpp) over its life: the calls that stage M points give the
same bits whether their buffers are fresh, have just been regrown for a larger M, or are reused at a smaller M than
they hold -- and again in a context whose buffers come, zeroed, out of the cache the closed contexts left.

A flat Bernoulli GLMTarget with n = 65 rows (two observation tiles) and p = 2, 64 resident particles.  M = 64 fits the
staging buffer smcn_ctx_create makes; M = 130 (three particle chunks, the last ragged) makes stage, pw.buf, ps.buf,
dr.buf, sm.buf and cov.buf regrow.  Every comparison is np.array_equal with NaNs compared by position."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, ROWS, P, M_NEW, S, SEED = 64, 65, 2, 3, 8, 20261019


def _case():
    import _pointwise as pw
    from smcnuts_amd import GLMTarget
    X, y = pw.synthetic("bernoulli_logit", ROWS, P, SEED)
    Xn, yn = pw.synthetic("bernoulli_logit", M_NEW, P, SEED + 1)
    t = GLMTarget(X, y, family="bernoulli_logit", prior_sd=np.array([0.8, 2.5]), intercept=False)
    block, has_y = t._predict_block(Xn, yn)
    return t, block, has_y


def _points(M):
    rng = np.random.default_rng(SEED + M)
    return 0.3 * rng.standard_normal((M, P)), 3.0 * rng.standard_normal(M)


def _round(ctx, M, block, has_y):
    """Every staged call once at M points -> {name: array}"""
    x, lw = _points(M)
    out = {"pointwise_partials": ctx.pointwise_partials(x, lw)}
    out["psis_loo"], out["psis_loo head"] = ctx.psis_loo(x, lw)
    ctx.predict_set_data(block, has_y)
    out["predict_partials"] = ctx.predict_partials(x, lw)
    y, anc, n_bad = ctx.predict_draws(S, SEED, x, lw)
    out["predict_draws"], out["predict_draws ancestors"], out["predict_draws n_bad"] = y, anc, np.array(n_bad)
    head, Dc = ctx.summary_begin(x, lw)
    out["summary_begin"] = head
    out["cov_partials"], out["cov_partials centre"] = ctx.cov_partials(head[0], Dc)
    out["target_eval"] = ctx.target_eval(x)[0]
    return out


def _same(got, want, what):
    assert list(got) == list(want)
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        eq = np.array_equal(g, w, equal_nan=True) if w.dtype.kind == "f" else np.array_equal(g, w)
        assert eq, f"{what}: {name} differs from the fresh context's"


def test_regrown_and_reused_buffers_give_the_fresh_context_s_bits():
    from smcnuts_amd import _capi
    t, block, has_y = _case()
    new = lambda: _capi.Context(N, t.model_id, t.model_data)
    fresh = {}
    for M in (64, 130):
        c = new()
        fresh[M] = _round(c, M, block, has_y)
        c.close()
    assert fresh[64]["pointwise_partials"].shape[0] == 1 + ROWS and fresh[130]["predict_draws"].shape == (S, M_NEW)
    ctx = new()
    for step, M in enumerate((64, 130, 64)):
        _same(_round(ctx, M, block, has_y), fresh[M], f"call {step} (M = {M})")
    ctx.close()
    again = new()                                    # (its buffers: the closed contexts', out of the cache)
    x, lw = _points(64)
    _same({"pointwise_partials": again.pointwise_partials(x, lw)},
          {"pointwise_partials": fresh[64]["pointwise_partials"]}, "after close")
    again.close()
