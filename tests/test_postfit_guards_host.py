"""Characterisation of what SMCSampler's eight post-fit methods (pointwise, loo, summary, covariance, predict,
predict_draws, forecast, forecast_draws) refuse before they reach the device, and in which order, against
tests/postfit_guards_expected.json, recorded from the code BEFORE the methods' guards were folded into shared helpers.
The file holds, per case, the exception's class with its whole message.

No device: the sampler is object.__new__(SMCSampler) with only the attributes the guards read (lkernel, target,
_finalised, phi, K, mean_estimate, rng, seed, a comm of one rank) and real targets built on the host; its `samples` is a
tripwire whose ctx raises ReachedDevice, which only the fault-free case "<method>/0/none" may record.

The table per method: the fault-free case; one case per fault, in the order the method checks them (the asymptotic
L-kernel; a target the product is not implemented for; a GLMTarget fitted with weights; a bad argument; not finalised;
phi[K] = 0.5); and, for every two faults adjacent in that order, the case with both, which records WHICH of the two is
reported.  (An unsupported target and a weighted GLMTarget are both "the target": they cannot be combined, so the pair
on either side of them is taken with each.)

    python tests/test_postfit_guards_host.py [ROOT]     rewrites the file from the package under ROOT (default: this tree)
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "postfit_guards_expected.json")


class ReachedDevice(Exception):
    pass


class _Tripwire:
    @property
    def ctx(self):
        raise ReachedDevice("the guards passed")


class _OneRank:
    world_size, rank = 1, 0


X = (np.arange(12, dtype=np.float64).reshape(6, 2) % 7.0 - 3.0) / 4.0
Y01 = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
WTS = np.array([1.0, 2.0, 0.0, 0.5, 3.0, 1.0])


def _sampler(S, target):
    s = object.__new__(S.SMCSampler)
    s.lkernel, s.target, s._finalised, s.K = "forwardsLKernel", target, True, 3
    s.phi = np.array([0.0, 0.3, 0.7, 1.0])
    s.mean_estimate = np.zeros((4, getattr(target, "constrained_dim", target.dim)))
    s.rng, s.seed, s.comm, s.samples = None, 1234, _OneRank(), _Tripwire()
    return s


# a fault changes the sampler `s` or the call's keywords `kw`
def _asymptotic(s, kw):
    s.lkernel = "asymptoticLKernel"


def _not_finalised(s, kw):
    s._finalised = False


def _phi_half(s, kw):
    s.phi = np.array([0.0, 0.2, 0.4, 0.5])


def _target(make):
    def f(s, kw):
        s.target = make()
        s.mean_estimate = np.zeros((4, s.target.constrained_dim))
    return f


def _arg(**kv):
    return lambda s, kw: kw.update(kv)


def _methods(T):
    """method -> (the fitted target, the call's keywords, [[(label, fault), ..] per position in the order of checks])."""
    glm = lambda: T.GLMTarget(X, Y01)                                   # noqa: E731
    gauss = ("target", _target(lambda: T.GaussianTarget(3)))
    weighted = ("weighted", _target(lambda: T.GLMTarget(X, Y01, weights=WTS)))
    first, last = [("asymptotic", _asymptotic)], [[("not_finalised", _not_finalised)], [("phi", _phi_half)]]
    Xn = X[:3] + 0.125
    return {
        "pointwise": (glm, {}, [first, [gauss, weighted]] + last),
        "loo": (glm, {}, [first, [gauss, weighted]] + last),
        "summary": (glm, {}, [first, [("probs", _arg(probs=[2.0]))]] + last),
        "covariance": (glm, {}, [first] + last),
        "predict": (glm, dict(X_new=Xn), [first, [gauss], [("X_new", _arg(X_new=np.zeros((3, 3))))]] + last),
        "predict_draws": (glm, dict(n_draws=4), [first, [gauss], [("n_draws", _arg(n_draws=0))]] + last),
        "forecast": (T.ArmaModel, dict(horizon=3), [first, [gauss], [("horizon", _arg(horizon=0))]] + last),
        "forecast_draws": (T.ArmaModel, dict(horizon=3, n_draws=4), [first, [gauss], [("horizon", _arg(horizon=0))]] + last),
    }


def build_cases(S, T):
    """case id -> a call that builds the sampler, applies the faults and runs the method."""
    cases = {}
    for method, (make, base, order) in _methods(T).items():
        def add(cid, *faults, method=method, make=make, base=base):
            def call():
                s, kw = _sampler(S, make()), dict(base)
                for f in faults:
                    f(s, kw)
                return getattr(s, method)(**kw)
            assert cid not in cases, cid
            cases[cid] = call
        add(f"{method}/0/none")
        for pos in order:
            for label, f in pos:
                add(f"{method}/1/{label}", f)
        for pos0, pos1 in zip(order, order[1:]):
            for l0, f0 in pos0:
                for l1, f1 in pos1:
                    add(f"{method}/2/{l0}+{l1}", f0, f1)
    return cases


def _outcome(call):
    try:
        call()
    except Exception as e:      # noqa: BLE001 -- the class is what is recorded
        return {"raises": type(e).__name__, "message": str(e)}
    return {"returns": True}


def record(S, T):
    return {cid: _outcome(call) for cid, call in build_cases(S, T).items()}


# ---- the tests -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    from smcnuts_amd import smc_sampler as S
    from smcnuts_amd.model import targets as T
    with open(EXPECTED) as f:
        return build_cases(S, T), json.load(f)


def test_the_file_holds_exactly_the_table(table):
    cases, want = table
    assert sorted(cases) == sorted(want)


@pytest.mark.parametrize("method", ["pointwise", "loo", "summary", "covariance", "predict", "predict_draws", "forecast",
                                    "forecast_draws"])
def test_every_case_does_what_it_did(table, method):
    cases, want = table
    wrong = {}
    for cid, call in cases.items():
        if cid.split("/")[0] == method:
            got = _outcome(call)
            if got != want[cid]:
                wrong[cid] = dict(got=got, want=want[cid])
    assert not wrong, json.dumps(wrong, indent=1)[:6000]


def test_only_the_fault_free_cases_reach_the_device(table):
    _, want = table
    for cid, w in want.items():
        assert "raises" in w, (cid, w)
        assert (w["raises"] == "ReachedDevice") == cid.endswith("/0/none"), (cid, w)


def test_a_single_fault_reports_itself(table):
    """The recorded table is the parent's; these are the texts the issue of the shared guards fixed, spelled out."""
    _, want = table
    for m, noun in (("pointwise", "criteria"), ("loo", "criteria"), ("summary", "summaries"), ("covariance", "covariances"),
                    ("predict", "predictions"), ("predict_draws", "predictions"), ("forecast", "forecasts"),
                    ("forecast_draws", "forecasts")):
        assert want[f"{m}/1/asymptotic"] == {"raises": "NotImplementedError", "message": (
            f"{m}(): the asymptotic L-kernel's estimates pool generations; {noun} over the pooled generations are not "
            "implemented")}
        assert want[f"{m}/1/not_finalised"] == {"raises": "RuntimeError", "message": (
            f"{m}(): run sample() (or step() K times and finalise()) first")}
        assert want[f"{m}/1/phi"] == {"raises": "RuntimeError", "message": (
            f"{m}(): the final temperature is phi = 0.5, not 1: the particles do not target the posterior")}
        assert want[f"{m}/2/not_finalised+phi"] == want[f"{m}/1/not_finalised"]


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(HERE))
    from smcnuts_amd import smc_sampler
    from smcnuts_amd.model import targets
    out = record(smc_sampler, targets)
    with open(EXPECTED, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    print(f"{len(out)} cases from {os.path.dirname(os.path.dirname(targets.__file__))} -> {EXPECTED}")
