"""The multilevel GLM's data block (SMCN_MODEL_MLGLM) through smcn_regdata.hpp's reg_check / reg_repack, under the
address and undefined-behaviour sanitizers.

tests/regdata_driver.cpp -- unchanged, a stand-alone program that includes only the header -- is compiled with
`g++ -fsanitize=address,undefined -fno-sanitize-recover=all` as tests/test_regdata_host.py compiles it and run once over
model-8 cases: every refusal of the model's Spec, accepted blocks for R = 1..4 at, one short of and one past their exact
length, and the repacked image bit for bit against `image`, a restatement of the layout in Python.  Every block is a
heap array of exactly its length, so a read past a caller-supplied length fails the run."""
import ctypes
import ctypes.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_regdata_host as rh

ROOT = rh.ROOT
MLGLM = 8
NAN, INF = float("nan"), float("inf")
WHO = "multilevel GLM target: "

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]


def block(rng, fam, n, p, ic, Js):
    """A valid block and its parts"""
    R, Dc = len(Js), p + ic
    head = [fam, n, p, ic, R] + list(Js) + [0] * (4 - R)
    pri = rh._sds(rng, Dc) + [0.75 + 0.25 * r for r in range(R)] + ([rh._grid(rng, 1)[0], 1.5] if fam >= 2 else [])
    y = rh._y(rng, fam, n)
    gz = []
    for J in Js:
        gz += rng.integers(0, J, size=n).astype(float).tolist() + rh._grid(rng, n)
    return [float(v) for v in head + pri + y + gz + rh._grid(rng, n * p)]


def offsets(b):
    fam, n, p, ic, R = (int(v) for v in b[:5])
    Dc = p + ic
    npri = Dc + R + (2 if fam >= 2 else 0)
    y0 = 9 + npri
    g0 = y0 + n
    X0 = y0 + (1 + 2 * R) * n
    return fam, n, p, ic, R, Dc, npri, y0, g0, X0, X0 + n * p


def image(b):
    """The repacked image and the 21 integers the driver prints, restated from the layout's description: the block, zeros
    to a 128-byte boundary, rows [1, X_i.., 0 to an even count DP, y_i, lgamma(y_i + 1) (0 for normal), g_1i, z_1i, ..,
    g_Ri, z_Ri] up to a multiple of 64."""
    fam, n, p, ic, R, Dc, npri, y0, g0, X0, ln = offsets(b)
    assert len(b) == ln
    Js = [int(v) for v in b[5:5 + R]]
    D = Dc + sum(Js) + R + (1 if fam >= 2 else 0)
    t0 = (ln + 15) // 16 * 16
    DP = (Dc + 1) // 2 * 2
    RS = DP + 2 + 2 * R
    rows = (n + 63) // 64 * 64
    img = np.zeros(t0 + rows * RS)
    img[:ln] = b
    for i in range(n):
        row = img[t0 + i * RS:t0 + (i + 1) * RS]
        if ic:
            row[0] = 1.0
        row[ic:ic + p] = b[X0 + i * p:X0 + (i + 1) * p]
        y = b[y0 + i]
        row[DP] = y
        row[DP + 1] = 0.0 if fam == 2 else _libm.lgamma(y + 1.0)
        for r in range(R):
            row[DP + 2 + 2 * r] = b[g0 + 2 * r * n + i]
            row[DP + 3 + 2 * r] = b[g0 + (2 * r + 1) * n + i]
    ints = [MLGLM, fam, 0, n, p, sum(Js), ic, Dc, D, 9, npri, y0, g0, X0, ln, t0, rows, RS, DP, 0, t0 + rows * RS]
    return img, ints


def cases():
    """[(name, block, expected message, or None for an accepted block)]"""
    rng = np.random.default_rng(20261019)
    out = []
    layout = WHO + "data = [family, n, p, intercept, R, J_1, J_2, J_3, J_4 (0 beyond R)"
    # accepted: R = 1..4, every family, n either side of the 64-row padding, both parities of Dc, Dc = 0
    shapes = [(0, 1, 0, 0, (1,)), (1, 63, 1, 0, (3, 3)), (2, 64, 2, 1, (1, 5, 2)), (3, 65, 5, 0, (1, 5, 2, 3)),
              (2, 7, 0, 1, (4,)), (0, 130, 3, 1, (2, 2, 2, 2))]
    for fam, n, p, ic, Js in shapes:
        b = block(rng, fam, n, p, ic, Js)
        tag = f"f{fam}-n{n}-p{p}-ic{ic}-R{len(Js)}"
        out.append((f"ok-{tag}", b, None))
        out.append((f"short-{tag}", b[:-1], layout))
        out.append((f"long-{tag}", b + [0.0], layout))
    # D = 64 accepted, D = 65 refused
    too_big = WHO + "the device functor covers D = Dc + J_1 + .. + J_R + R (+ 1) <= 64 coordinates; larger models run " \
        "host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target"
    b = block(rng, 0, 2, 4, 1, (18, 18, 20))
    out.append(("D64", b, None))
    out.append(("D65", rh._with(b, 7, 21.0), too_big))
    b = block(rng, 3, 2, 3, 1, (18, 18, 20))
    out.append(("D64-disp", b, None))
    out.append(("D65-disp", rh._with(b, 2, 4.0), too_big))
    # refusals, from one small valid block per family (R = 2, p = 2, intercept: Dc = 3, n = 3)
    base = {fam: block(rng, fam, 3, 2, 1, (2, 3)) for fam in range(4)}
    Dc, R, n = 3, 2, 3

    def bad(tag, fam, b, msg):
        out.append((f"bad-f{fam}-{tag}", [float(v) for v in b], msg if msg.startswith(WHO) else WHO + msg))

    for fam, b in base.items():
        _, _, _, _, _, _, _, y0, g0, X0, ln = offsets(b)
        bad("len-header", fam, b[:8], layout)
        bad("len-one", fam, b[:1], layout)
        bad("header-only", fam, b[:9], layout)
        for tag, v in (("four", 4.0), ("half", 0.5), ("neg", -1.0), ("nan", NAN)):
            bad(f"fam-{tag}", fam, rh._with(b, 0, v), "family must be 0 (bernoulli_logit), 1 (poisson_log), 2 (normal) or 3 "
                "(neg_binomial_2_log)")
        for tag, v in (("two", 2.0), ("half", 0.5), ("nan", NAN)):
            bad(f"ic-{tag}", fam, rh._with(b, 3, v), "intercept must be 0 or 1")
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 2147483648.0), ("nan", NAN)):
            bad(f"n-{tag}", fam, rh._with(b, 1, v), "n must be an integer >= 1")
        for tag, v in (("neg", -1.0), ("frac", 0.5), ("big", 1048577.0), ("inf", INF)):
            bad(f"p-{tag}", fam, rh._with(b, 2, v), "p must be an integer >= 0")
        for tag, v in (("zero", 0.0), ("five", 5.0), ("frac", 1.5), ("nan", NAN), ("neg", -1.0)):
            bad(f"R-{tag}", fam, rh._with(b, 4, v), "R must be an integer in [1, 4] (the number of varying terms)")
        jmsg = "J_r must be an integer >= 1 (the levels of term r) for r <= R and 0 beyond R"
        for tag, q, v in (("zero", 5, 0.0), ("frac", 6, 2.5), ("big", 5, 1048577.0), ("nan", 6, NAN), ("beyond", 7, 1.0),
                          ("beyond-last", 8, 3.0), ("beyond-nan", 8, NAN)):
            bad(f"J-{tag}", fam, rh._with(b, q, v), jmsg)
        for tag, q, v in (("first-zero", 9, 0.0), ("last-inf", 9 + Dc - 1, INF), ("first-nan", 9, NAN)):
            bad(f"sd-{tag}", fam, rh._with(b, q, v), "prior sds must be finite and > 0")
        for tag, q, v in (("1-zero", 9 + Dc, 0.0), ("2-nan", 9 + Dc + 1, NAN), ("2-inf", 9 + Dc + 1, INF)):
            bad(f"s_tau-{tag}", fam, rh._with(b, q, v), "s_tau must be finite and > 0")
        if fam >= 2:
            bad("m_d-nan", fam, rh._with(b, 9 + Dc + R, NAN), "m_d must be finite")
            bad("m_d-inf", fam, rh._with(b, 9 + Dc + R, -INF), "m_d must be finite")
            bad("s_d-zero", fam, rh._with(b, 10 + Dc + R, 0.0), "s_d must be finite and > 0")
            bad("s_d-inf", fam, rh._with(b, 10 + Dc + R, INF), "s_d must be finite and > 0")
        ys, ymsg = {0: ((2.0, 0.5, -1.0, NAN), "bernoulli_logit needs y in {0, 1}"),
                    1: ((-1.0, 0.5, INF, NAN, 2.0 ** 54), "poisson_log needs y in {0, 1, 2, ..}"),
                    2: ((INF, -INF, NAN), "normal needs finite y"),
                    3: ((-1.0, 0.5, 2.0 ** 54, NAN), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}")}[fam]
        for j, v in enumerate(ys):
            bad(f"y-{j}", fam, rh._with(b, y0 + j % n, v), ymsg)
        gmsg = "every group index g_r must be an integer in [0, J_r)"
        for tag, q, v in (("1-neg", g0, -1.0), ("1-J", g0 + 1, 2.0), ("1-frac", g0 + 2, 0.5), ("1-nan", g0, NAN),
                          ("2-J", g0 + 2 * n + 1, 3.0), ("2-inf", g0 + 2 * n + 2, INF)):
            bad(f"g-{tag}", fam, rh._with(b, q, v), gmsg)
        for tag, q, v in (("1-nan", g0 + n, NAN), ("2-inf", g0 + 3 * n + 2, -INF)):
            bad(f"z-{tag}", fam, rh._with(b, q, v), "z must be finite")
        bad("X-nan", fam, rh._with(b, ln - 1, NAN), "X must be finite")
        bad("X-inf", fam, rh._with(b, X0, -INF), "X must be finite")
    out.append(("ok-f3-y-2^53", rh._with(base[3], offsets(base[3])[7], 2.0 ** 53), None))   # (the bound is inclusive)
    return out


# the model's Spec texts and the shared refusals: each at least once
N_MESSAGES = 19


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/regdata_driver.cpp"
    tmp = str(tmp_path_factory.mktemp("mlglm_regdata"))
    exe = os.path.join(tmp, "regdata_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "regdata_driver.cpp"), "-o", exe])
    cs = cases()
    path = os.path.join(tmp, "cases.txt")
    rh.write_cases(path, [(name, MLGLM, b, None) for name, b, _ in cs])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stderr[-4000:]}"
    res = rh.parse(r.stdout)
    assert list(res) == [c[0] for c in cs], "the driver did not print every case once"
    return res


def test_cases_name_every_refusal():
    cs = cases()
    assert len({name for name, _, _ in cs}) == len(cs)
    assert len({msg for _, _, msg in cs if msg}) == N_MESSAGES
    assert {int(b[4]) for _, b, msg in cs if msg is None} == {1, 2, 3, 4}


def test_refusals_and_images_under_sanitizers(driver_output):
    for name, b, msg in cases():
        got = driver_output[name]
        if msg is not None:
            assert got["msg"].startswith(msg), (name, got["msg"], msg)
            assert list(got) == ["msg"], name
            continue
        assert got["msg"] == "", (name, got["msg"])
        img, ints = image(np.array(b, dtype=np.float64))
        assert got["ints"].tolist() == ints, (name, got["ints"].tolist(), ints)
        gv = got["vec"]
        assert gv.shape == img.shape and (gv.view(np.int64) == img.view(np.int64)).all(), name
