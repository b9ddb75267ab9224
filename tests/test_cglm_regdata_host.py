"""The continuous GLM's data block (SMCN_MODEL_CGLM) through smcn_regdata.hpp's reg_check / reg_repack, under the address
and undefined-behaviour sanitizers.

tests/regdata_driver.cpp -- unchanged, a stand-alone program with its own main that includes only the header -- is
compiled with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` as tests/test_regdata_host.py compiles it and
run once over model-12 cases: accepted blocks for both families x (p, intercept) giving odd and even row widths with and
without the intercept x n in {1, 63, 64, 65} (their repacked image bit for bit against `image`, a restatement of the
layout in Python), and every refusal with its text.  Every block is a heap array of exactly its length, so a read past a
caller-supplied length fails the run."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_regdata_host as rh

ROOT = rh.ROOT
CGLM = 12
NAN, INF = float("nan"), float("inf")
WHO = "continuous GLM target: "
N_LIST = (1, 63, 64, 65)
SHAPES = ((2, 1), (3, 1), (2, 0), (3, 0))          # (p, intercept): Dc = 3, 4, 2, 3


def block(rng, fam, n, p, ic, df=None):
    Dc = p + ic
    y = (rng.integers(1, 40, size=n) / 8.0).tolist() if fam == 0 else rh._grid(rng, n)
    dfv = 0.0 if fam == 0 else (rng.choice([0.5, 1.0, 4.0, 30.0]) if df is None else df)
    return [float(fam), float(n), float(p), float(ic), float(dfv)] + rh._sds(rng, Dc) + [0.25, 1.5] + y + rh._grid(rng, n * p)


def image(b):
    """The repacked image and the 21 integers the driver prints, restated from the layout's description: the block, zeros
    to the 128-byte boundary, rows [1 (intercept), X_i.., 0 to an even count DP, y_i, log y_i (gamma_log) or 0], zero rows
    up to a multiple of 64."""
    fam, n, p, ic = (int(v) for v in b[:4])
    Dc = p + ic
    npri = Dc + 2
    y0 = 5 + npri
    X0 = y0 + n
    ln = X0 + n * p
    assert len(b) == ln
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
        row[DP] = b[y0 + i]
        row[DP + 1] = math.log(b[y0 + i]) if fam == 0 else 0.0
    return img, [CGLM, fam, 0, n, p, 0, ic, Dc, Dc + 1, 5, npri, y0, 0, X0, ln, t0, rows, RS, DP, 0, t0 + rows * RS]


LAYOUT = WHO + "data = [family, n, p, intercept, df, s_1..s_Dc, m_tau, s_tau, y_1..y_n, X (n x p, row-major)]"
TOO_BIG = WHO + "the device functor covers D = Dc + 1 <= 64 coordinates (the coefficients and tau); larger models run " \
    "host-evaluated (SMCN_MODEL_HOST + smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)"
FAMILY = "family must be 0 (gamma_log) or 1 (student_t)"
Y_GAMMA = "gamma_log needs finite y > 0 (a zero has no gamma density: model zeros apart)"


def cases():
    """[(name, block, expected message, or None for an accepted block)]"""
    rng = np.random.default_rng(20261021)
    out = []
    for fam in (0, 1):
        for p, ic in SHAPES:
            for n in N_LIST:
                out.append((f"ok-f{fam}-p{p}-ic{ic}-n{n}", block(rng, fam, n, p, ic), None))
        b = block(rng, fam, 2, 62, 1)                       # D = 64
        out.append((f"D64-f{fam}", b, None))
        out.append((f"D65-f{fam}-header", rh._with(b, 2, 63.0), TOO_BIG))
        out.append((f"D65-f{fam}-block", block(rng, fam, 2, 63, 1), TOO_BIG))
        out.append((f"D65-f{fam}-no-intercept", block(rng, fam, 2, 64, 0), TOO_BIG))
    out.append(("ok-y-tiny-and-huge", rh._with(rh._with(block(rng, 0, 3, 2, 1), 5 + 5, 1e-300), 5 + 6, 1e300), None))
    base = {fam: block(rng, fam, 3, 4, 1) for fam in (0, 1)}         # Dc = 5, n = 3
    Dc, n = 5, 3
    y0, X0 = 5 + Dc + 2, 5 + Dc + 2 + n

    def bad(tag, fam, b, msg):
        out.append((f"bad-f{fam}-{tag}", [float(v) for v in b], msg if msg.startswith(WHO) else WHO + msg))

    for fam, b in base.items():
        bad("len-short", fam, b[:-1], LAYOUT)
        bad("len-long", fam, b + [0.0], LAYOUT)
        bad("header-only", fam, b[:5], LAYOUT)
        bad("len-header", fam, b[:4], LAYOUT)
        bad("len-one", fam, b[:1], LAYOUT)
        for tag, v in (("two", 2.0), ("three", 3.0), ("half", 0.5), ("neg", -1.0), ("nan", NAN)):
            bad(f"fam-{tag}", fam, rh._with(b, 0, v), FAMILY)
        for tag, v in (("two", 2.0), ("half", 0.5), ("nan", NAN)):
            bad(f"ic-{tag}", fam, rh._with(b, 3, v), "intercept must be 0 or 1")
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 2147483648.0), ("nan", NAN)):
            bad(f"n-{tag}", fam, rh._with(b, 1, v), "n must be an integer >= 1")
        for tag, v in (("neg", -1.0), ("frac", 3.5), ("big", 1048577.0), ("inf", INF)):
            bad(f"p-{tag}", fam, rh._with(b, 2, v), "p must be an integer >= 0")
        bad("no-cols", fam, rh._with(rh._with(b, 2, 0.0), 3, 0.0), "no coefficients (p = 0 without an intercept)")
        for tag, q, v in (("first-zero", 5, 0.0), ("last-inf", 5 + Dc - 1, INF), ("nan", 6, NAN), ("neg", 7, -1.0)):
            bad(f"sd-{tag}", fam, rh._with(b, q, v), "prior sds must be finite and > 0")
        bad("m_tau-nan", fam, rh._with(b, 5 + Dc, NAN), "m_tau must be finite")
        bad("m_tau-inf", fam, rh._with(b, 5 + Dc, -INF), "m_tau must be finite")
        for tag, v in (("zero", 0.0), ("inf", INF), ("nan", NAN), ("neg", -1.0)):
            bad(f"s_tau-{tag}", fam, rh._with(b, 6 + Dc, v), "s_tau must be finite and > 0")
        if fam == 0:
            for j, v in enumerate((0.0, -0.0, -1.0, INF, NAN, -INF)):
                bad(f"y-{j}", fam, rh._with(b, y0 + j % n, v), Y_GAMMA)
            for tag, v in (("four", 4.0), ("neg", -1.0), ("nan", NAN), ("inf", INF)):
                bad(f"df-{tag}", fam, rh._with(b, 4, v), "gamma_log has no df: the slot must be 0")
        else:
            for j, v in enumerate((INF, -INF, NAN)):
                bad(f"y-{j}", fam, rh._with(b, y0 + j, v), "student_t needs finite y")
            for tag, v in (("zero", 0.0), ("neg", -4.0), ("nan", NAN), ("inf", INF)):
                bad(f"df-{tag}", fam, rh._with(b, 4, v), "student_t needs df finite and > 0")
        bad("X-nan", fam, rh._with(b, len(b) - 1, NAN), "X must be finite")
        bad("X-inf", fam, rh._with(b, X0, -INF), "X must be finite")
    return out


# the Spec's texts (layout, family, too big, sds), the shared refusals (intercept, n, p, no coefficients, m_tau, s_tau, X)
# and the model's own (two y texts, two df texts)
N_MESSAGES = 15


@pytest.fixture(scope="module")
def driver_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/regdata_driver.cpp"
    exe = os.path.join(str(tmp_path_factory.mktemp("cglm_regdata")), "regdata_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "regdata_driver.cpp"), "-o", exe])
    return exe


def _run(exe, cs):
    path = os.path.join(os.path.dirname(exe), f"cases{len(cs)}.txt")
    rh.write_cases(path, cs)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stderr[-4000:]}"
    res = rh.parse(r.stdout)
    assert list(res) == [c[0] for c in cs], "the driver did not print every case once"
    return res


@pytest.fixture(scope="module")
def driver_output(driver_exe):
    return _run(driver_exe, [(name, CGLM, b, None) for name, b, _ in cases()])


def test_cases_name_every_refusal_and_shape():
    cs = cases()
    assert len({name for name, _, _ in cs}) == len(cs)
    assert len({msg for _, _, msg in cs if msg}) == N_MESSAGES
    ok = {(int(b[0]), int(b[2]), int(b[3]), int(b[1])) for _, b, msg in cs if msg is None}
    assert {(f, p, ic, n) for f in (0, 1) for p, ic in SHAPES for n in N_LIST} <= ok
    assert {(p + ic) % 2 for p, ic in SHAPES} == {0, 1} and {ic for _, ic in SHAPES} == {0, 1}


def test_refusals_and_images_under_sanitizers(driver_output):
    for name, b, msg in cases():
        got = driver_output[name]
        if msg is not None:
            assert got["msg"] == msg, (name, got["msg"], msg)
            assert list(got) == ["msg"], name
            continue
        assert got["msg"] == "", (name, got["msg"])
        img, ints = image(np.array(b, dtype=np.float64))
        assert got["ints"].tolist() == ints, (name, got["ints"].tolist(), ints)
        gv = got["vec"]
        assert gv.shape == img.shape and (gv.view(np.int64) == img.view(np.int64)).all(), name


def test_other_ids_do_not_take_the_block_and_id_11_is_no_regression_model(driver_exe):
    """The new block under SMCN_MODEL_GLM's id is refused by that id's own checks, never read past; the plain block under
    id 12 likewise; id 11 stays unassigned."""
    rng = np.random.default_rng(5)
    mine, plain = block(rng, 1, 4, 2, 1, df=4.0), rh.block(rng, rh.GLM, 2, 4, 2, 1)
    res = _run(driver_exe, [("mine-as-4", rh.GLM, mine, None), ("plain-as-12", CGLM, plain, None),
                            ("plain-as-4", rh.GLM, plain, None), ("mine-as-11", 11, mine, None)])
    assert res["mine-as-4"]["msg"].startswith("GLM target: ")
    assert res["plain-as-12"]["msg"].startswith(WHO)
    assert res["plain-as-4"]["msg"] == ""
    assert res["mine-as-11"]["msg"] == "not a regression model"
