"""The wide GLM's data block (SMCN_MODEL_WGLM) through smcn_regdata.hpp's reg_check / reg_repack, under the address and
undefined-behaviour sanitizers.

tests/regdata_driver.cpp -- unchanged, a stand-alone program that includes only the header -- is compiled with
`g++ -fsanitize=address,undefined -fno-sanitize-recover=all` as tests/test_regdata_host.py compiles it and run once over
model-9 cases: accepted blocks for D in {65, 128, 129, 256} x n in {1, 63, 64, 65} x the four families (their repacked
image bit for bit against `image`, a restatement of the layout in Python), and every refusal of the model's Spec with its
text.  Every block is a heap array of exactly its length, so a read past a caller-supplied length fails the run."""
import ctypes
import ctypes.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_regdata_host as rh

ROOT = rh.ROOT
WGLM = 9
NAN, INF = float("nan"), float("inf")
WHO = "wide GLM target: "
D_LIST, N_LIST = (65, 128, 129, 256), (1, 63, 64, 65)

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]


def block(rng, fam, n, p, ic):
    """A valid block: SMCN_MODEL_GLM's layout"""
    return rh.block(rng, rh.GLM, fam, n, p, ic)


def offsets(b):
    fam, n, p, ic = (int(v) for v in b[:4])
    Dc = p + ic
    npri = Dc + (2 if fam >= 2 else 0)
    y0 = 4 + npri
    X0 = y0 + n
    return fam, n, p, ic, Dc, npri, y0, X0, X0 + n * p


def image(b):
    """The repacked image and the 21 integers the driver prints, restated from the layout's description: the block, zeros
    to a 128-byte boundary, rows [1 (intercept), X_i.., 0 to an even count DP, y_i, lgamma(y_i + 1) (0 for normal)], zero
    rows up to a multiple of 64."""
    fam, n, p, ic, Dc, npri, y0, X0, ln = offsets(b)
    assert len(b) == ln
    D = Dc + (1 if fam >= 2 else 0)
    t0 = (ln + 15) // 16 * 16
    DP = (Dc + 1) // 2 * 2
    RS = DP + 2
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
    ints = [WGLM, fam, 0, n, p, 0, ic, Dc, D, 4, npri, y0, 0, X0, ln, t0, rows, RS, DP, 0, t0 + rows * RS]
    return img, ints


TOO_SMALL = WHO + "the device functor covers 65 <= D <= 256 coordinates (D counts tau for families 2 and 3); D <= 64 is " \
    "SMCN_MODEL_GLM's (GLMTarget)"
TOO_BIG = WHO + "the device functor covers 65 <= D <= 256 coordinates; larger models run host-evaluated (SMCN_MODEL_HOST + " \
    "smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)"


def cases():
    """[(name, block, expected message, or None for an accepted block)]"""
    rng = np.random.default_rng(20261020)
    out = []
    layout = WHO + "data = [family, n, p, intercept, s_1..s_D, y_1..y_n, X (n x p, row-major)]"
    k = 0
    for fam in range(4):
        for D in D_LIST:
            for n in N_LIST:
                ic = k % 2                                  # (both layouts of the row; D counts tau for families 2, 3)
                k += 1
                p = D - ic - (1 if fam >= 2 else 0)
                out.append((f"ok-f{fam}-D{D}-n{n}-ic{ic}", block(rng, fam, n, p, ic), None))
    # the bounds, from a header alone (the refusal comes before the length check) and from whole blocks
    for fam in range(4):
        t = 1 if fam >= 2 else 0
        b = block(rng, fam, 2, 64 - t, 1)                   # D = 65
        out.append((f"D65-f{fam}", b, None))
        out.append((f"D64-f{fam}-header", rh._with(b, 2, 63.0 - t), TOO_SMALL))
        out.append((f"D64-f{fam}-noic", rh._with(b, 3, 0.0), TOO_SMALL))
        out.append((f"D64-f{fam}-block", block(rng, fam, 2, 63 - t, 1), TOO_SMALL))
        out.append((f"D1-f{fam}", block(rng, fam, 2, 1, 0), TOO_SMALL))
        b = block(rng, fam, 2, 255 - t, 1)                  # D = 256
        out.append((f"D256-f{fam}", b, None))
        out.append((f"D257-f{fam}-header", rh._with(b, 2, 256.0 - t), TOO_BIG))
        out.append((f"D257-f{fam}-block", block(rng, fam, 2, 256 - t, 1), TOO_BIG))
        out.append((f"D1048577-f{fam}", rh._with(b, 2, 1048576.0), TOO_BIG))
    # refusals, from one valid block per family (p = 65, intercept: Dc = 66, n = 3)
    base = {fam: block(rng, fam, 3, 65, 1) for fam in range(4)}
    Dc, n = 66, 3

    def bad(tag, fam, b, msg):
        out.append((f"bad-f{fam}-{tag}", [float(v) for v in b], msg if msg.startswith(WHO) else WHO + msg))

    for fam, b in base.items():
        _, _, _, _, _, _, y0, X0, ln = offsets(b)
        disp_layout = "data = [family, n, p, intercept, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, row-major)] for " \
            "families 2 (normal) and 3 (neg_binomial_2_log)"
        short = disp_layout if fam >= 2 else layout
        bad("len-short", fam, b[:-1], short)
        bad("len-long", fam, b + [0.0], short)
        bad("header-only", fam, b[:4], short)
        bad("len-header", fam, b[:3], layout)
        bad("len-one", fam, b[:1], layout)
        for tag, v in (("four", 4.0), ("half", 0.5), ("neg", -1.0), ("nan", NAN)):
            bad(f"fam-{tag}", fam, rh._with(b, 0, v), "family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) "
                "or 3 (neg_binomial_2_log) with a dispersion prior")
        for tag, v in (("two", 2.0), ("half", 0.5), ("nan", NAN)):
            bad(f"ic-{tag}", fam, rh._with(b, 3, v), "intercept must be 0 or 1")
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 2147483648.0), ("nan", NAN)):
            bad(f"n-{tag}", fam, rh._with(b, 1, v), "n must be an integer >= 1")
        for tag, v in (("neg", -1.0), ("frac", 64.5), ("big", 1048577.0), ("inf", INF)):
            bad(f"p-{tag}", fam, rh._with(b, 2, v), "p must be an integer >= 0")
        bad("no-cols", fam, rh._with(rh._with(b, 2, 0.0), 3, 0.0), "no coefficients (p = 0 without an intercept)")
        for tag, q, v in (("first-zero", 4, 0.0), ("last-inf", 4 + Dc - 1, INF), ("slot1-nan", 4 + 64, NAN),
                          ("slot1-neg", 4 + 65, -1.0)):
            bad(f"sd-{tag}", fam, rh._with(b, q, v), "prior sds must be finite and > 0")
        if fam >= 2:
            bad("m_tau-nan", fam, rh._with(b, 4 + Dc, NAN), "m_tau must be finite")
            bad("m_tau-inf", fam, rh._with(b, 4 + Dc, -INF), "m_tau must be finite")
            bad("s_tau-zero", fam, rh._with(b, 5 + Dc, 0.0), "s_tau must be finite and > 0")
            bad("s_tau-inf", fam, rh._with(b, 5 + Dc, INF), "s_tau must be finite and > 0")
            bad("laid-out-for-0-1", fam, b[:4 + Dc] + b[6 + Dc:], "family must be 0 (bernoulli_logit) or 1 (poisson_log) "
                "for a block without m_tau, s_tau; families 2 (normal) and 3 (neg_binomial_2_log) take data = [family, n, "
                "p, intercept, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X]")
        ys, ymsg = {0: ((2.0, 0.5, -1.0, NAN), "bernoulli_logit needs y in {0, 1}"),
                    1: ((-1.0, 0.5, INF, NAN, 2.0 ** 54), "poisson_log needs y in {0, 1, 2, ..}"),
                    2: ((INF, -INF, NAN), "normal needs finite y"),
                    3: ((-1.0, 0.5, 2.0 ** 54, NAN), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}")}[fam]
        for j, v in enumerate(ys):
            bad(f"y-{j}", fam, rh._with(b, y0 + j % n, v), ymsg)
        bad("X-nan", fam, rh._with(b, ln - 1, NAN), "X must be finite")
        bad("X-inf", fam, rh._with(b, X0, -INF), "X must be finite")
        bad("X-inf-slot1", fam, rh._with(b, X0 + 64, INF), "X must be finite")
    out.append(("ok-f3-y-2^53", rh._with(base[3], offsets(base[3])[6], 2.0 ** 53), None))   # (the bound is inclusive)
    return out


# the model's Spec texts (layout, family, too small, too big, sds), the two dispersion-family layouts and the shared
# refusals (intercept, n, p, no coefficients, m_tau, s_tau, four y texts, X): each at least once
N_MESSAGES = 18


@pytest.fixture(scope="module")
def driver_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/regdata_driver.cpp"
    exe = os.path.join(str(tmp_path_factory.mktemp("wglm_regdata")), "regdata_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "regdata_driver.cpp"), "-o", exe])
    return exe


def _run(exe, cs):
    """cs: [(name, model, block)] -> the driver's parsed output"""
    path = os.path.join(os.path.dirname(exe), f"cases{len(cs)}.txt")
    rh.write_cases(path, [(name, model, b, None) for name, model, b in cs])
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stderr[-4000:]}"
    res = rh.parse(r.stdout)
    assert list(res) == [c[0] for c in cs], "the driver did not print every case once"
    return res


@pytest.fixture(scope="module")
def driver_output(driver_exe):
    return _run(driver_exe, [(name, WGLM, b) for name, b, _ in cases()])


def test_cases_name_every_refusal_and_shape():
    cs = cases()
    assert len({name for name, _, _ in cs}) == len(cs)
    assert len({msg for _, _, msg in cs if msg}) == N_MESSAGES
    ok = {(int(b[0]), offsets(b)[4] + (1 if b[0] >= 2 else 0), int(b[1])) for _, b, msg in cs if msg is None}
    assert {(f, D, n) for f in range(4) for D in D_LIST for n in N_LIST} <= ok


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


def test_one_block_two_ids(driver_exe):
    """SMCN_MODEL_GLM keeps its own text for D = 65 and SMCN_MODEL_WGLM sends a D = 64 block there; where both layouts
    exist (the table is generic in D) the two ids repack a block into the same image."""
    rng = np.random.default_rng(5)
    b65, b64 = block(rng, 1, 2, 64, 1), block(rng, 1, 2, 63, 1)
    res = _run(driver_exe, [("glm65", rh.GLM, b65), ("glm64", rh.GLM, b64), ("wide64", WGLM, b64), ("wide65", WGLM, b65)])
    assert res["glm65"]["msg"].startswith("GLM target: the device functor covers D <= 64 coefficients; larger models run "
                                          "host-evaluated")
    assert res["wide64"]["msg"] == TOO_SMALL
    for name, b, model in (("glm64", b64, rh.GLM), ("wide65", b65, WGLM)):
        img, ints = image(np.array(b, dtype=np.float64))
        assert res[name]["msg"] == ""
        assert res[name]["ints"].tolist() == [model] + ints[1:]
        assert (res[name]["vec"].view(np.int64) == img.view(np.int64)).all()
