"""The offset / weights GLM's data block (SMCN_MODEL_OGLM) through smcn_regdata.hpp's reg_check / reg_repack /
reg_splice, under the address and undefined-behaviour sanitizers.

tests/regdata_driver.cpp -- unchanged, a stand-alone program with its own main that includes only the header -- is
compiled with `g++ -fsanitize=address,undefined -fno-sanitize-recover=all` as tests/test_regdata_host.py compiles it and
run once over model-10 cases: accepted blocks for flags {1, 2, 3} x the four families x (p, intercept) giving odd and
even row widths with and without the intercept x n in {1, 63, 64, 65} (their repacked image bit for bit against `image`,
a restatement of the layout in Python), new rows spliced behind the training priors, and every refusal with its text.
Every block is a heap array of exactly its length, so a read past a caller-supplied length fails the run."""
import ctypes
import ctypes.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_regdata_host as rh

ROOT = rh.ROOT
OGLM = 10
NAN, INF = float("nan"), float("inf")
WHO = "offset GLM target: "
N_LIST = (1, 63, 64, 65)
SHAPES = ((2, 1), (3, 1), (2, 0), (3, 0))          # (p, intercept): Dc = 3, 4, 2, 3

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]


def block(rng, fam, n, p, ic, flags, priors=True):
    """A valid block (priors=False: the new rows' block of smcn_predict_set_data, without them)"""
    b = rh.block(rng, rh.GLM, fam, n, p, ic)
    npri = p + ic + (2 if fam >= 2 else 0)
    o = rh._grid(rng, n) if flags & 1 else []
    w = (rng.integers(0, 9, size=n) / 4.0).tolist() if flags & 2 else []
    if w and not any(v > 0 for v in w):
        w[0] = 1.0
    return b[:4] + [float(flags)] + (b[4:4 + npri] if priors else []) + b[4 + npri:4 + npri + n] + o + w + b[4 + npri + n:]


def offsets(b):
    fam, n, p, ic, flags = (int(v) for v in b[:5])
    Dc = p + ic
    npri = Dc + (2 if fam >= 2 else 0)
    y0 = 5 + npri
    o0 = y0 + n if flags & 1 else 0
    w0 = y0 + (2 if flags & 1 else 1) * n if flags & 2 else 0
    X0 = y0 + (1 + (flags & 1) + (flags >> 1)) * n
    return fam, n, p, ic, flags, Dc, npri, y0, o0, w0, X0, X0 + n * p


def image(b):
    """The repacked image and the 21 integers the driver prints, restated from the layout's description: the block, zeros
    to the 128-byte boundary behind where a block with BOTH o and w would end, rows [1 (intercept), X_i.., 0 to an even
    count DP, y_i, lgamma(y_i + 1) (0 for normal), o_i (0 if absent), w_i (1 if absent)], zero rows up to a multiple of
    64."""
    fam, n, p, ic, flags, Dc, npri, y0, o0, w0, X0, ln = offsets(b)
    assert len(b) == ln
    D = Dc + (1 if fam >= 2 else 0)
    t0 = (5 + npri + 3 * n + n * p + 15) // 16 * 16
    DP = (Dc + 1) // 2 * 2
    RS = DP + 4
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
        row[DP + 2] = b[o0 + i] if o0 else 0.0
        row[DP + 3] = b[w0 + i] if w0 else 1.0
    ints = [OGLM, fam, 0, n, p, 0, ic, Dc, D, 5, npri, y0, 0, X0, ln, t0, rows, RS, DP, 0, t0 + rows * RS]
    return img, ints


LAYOUT = WHO + "data = [family, n, p, intercept, flags, s_1..s_D, y_1..y_n, o_1..o_n (flags & 1), w_1..w_n (flags & 2), " \
    "X (n x p, row-major)]"
DISP_LAYOUT = WHO + "data = [family, n, p, intercept, flags, s_1..s_Dc, m_tau, s_tau, y_1..y_n, o_1..o_n (flags & 1), " \
    "w_1..w_n (flags & 2), X (n x p, row-major)] for families 2 (normal) and 3 (neg_binomial_2_log)"
TOO_BIG = WHO + "the device functor covers D <= 64 coefficients; larger models run host-evaluated (SMCN_MODEL_HOST + " \
    "smcn_set_host_target: any object with logpdf / logpdfgrad through HostTarget)"
FLAGS0 = WHO + "flags = 0 (neither offsets nor weights) is SMCN_MODEL_GLM's model: pass the block without the flags slot " \
    "as SMCN_MODEL_GLM"


def cases():
    """[(name, block, expected message, or None for an accepted block)]"""
    rng = np.random.default_rng(20261019)
    out = []
    for flags in (1, 2, 3):
        for fam in range(4):
            for p, ic in SHAPES:
                for n in N_LIST:
                    out.append((f"ok-fl{flags}-f{fam}-p{p}-ic{ic}-n{n}", block(rng, fam, n, p, ic, flags), None))
    # the bound on D, from a header alone and from whole blocks
    for fam in range(4):
        t = 1 if fam >= 2 else 0
        b = block(rng, fam, 2, 63 - t, 1, 3)                # D = 64
        out.append((f"D64-f{fam}", b, None))
        out.append((f"D65-f{fam}-header", rh._with(b, 2, 64.0 - t), TOO_BIG))
        out.append((f"D65-f{fam}-block", block(rng, fam, 2, 64 - t, 1, 1), TOO_BIG))
    base = {fam: block(rng, fam, 3, 4, 1, 3) for fam in range(4)}     # Dc = 5, n = 3, both o and w
    Dc, n = 5, 3

    def bad(tag, fam, b, msg):
        out.append((f"bad-f{fam}-{tag}", [float(v) for v in b], msg if msg.startswith(WHO) else WHO + msg))

    for fam, b in base.items():
        _, _, _, _, _, _, _, y0, o0, w0, X0, ln = offsets(b)
        short = DISP_LAYOUT if fam >= 2 else LAYOUT
        bad("len-short", fam, b[:-1], short)
        bad("len-long", fam, b + [0.0], short)
        bad("header-only", fam, b[:5], short)
        bad("len-header", fam, b[:4], LAYOUT)
        bad("len-one", fam, b[:1], LAYOUT)
        bad("flags-zero", fam, rh._with(b, 4, 0.0), FLAGS0)
        for tag, v in (("four", 4.0), ("frac", 1.5), ("neg", -1.0), ("nan", NAN)):
            bad(f"flags-{tag}", fam, rh._with(b, 4, v), "flags must be 1 (offsets), 2 (weights) or 3 (both)")
        # (a block laid out for flags 3 under flags 1: the length says so)
        bad("flags-one-of-three", fam, rh._with(b, 4, 1.0), short)
        for tag, v in (("four", 4.0), ("half", 0.5), ("neg", -1.0), ("nan", NAN)):
            bad(f"fam-{tag}", fam, rh._with(b, 0, v), "family must be 0 (bernoulli_logit) or 1 (poisson_log), or 2 (normal) "
                "or 3 (neg_binomial_2_log) with a dispersion prior")
        for tag, v in (("two", 2.0), ("half", 0.5), ("nan", NAN)):
            bad(f"ic-{tag}", fam, rh._with(b, 3, v), "intercept must be 0 or 1")
        for tag, v in (("zero", 0.0), ("frac", 1.5), ("big", 2147483648.0), ("nan", NAN)):
            bad(f"n-{tag}", fam, rh._with(b, 1, v), "n must be an integer >= 1")
        for tag, v in (("neg", -1.0), ("frac", 3.5), ("big", 1048577.0), ("inf", INF)):
            bad(f"p-{tag}", fam, rh._with(b, 2, v), "p must be an integer >= 0")
        bad("no-cols", fam, rh._with(rh._with(b, 2, 0.0), 3, 0.0), "no coefficients (p = 0 without an intercept)")
        for tag, q, v in (("first-zero", 5, 0.0), ("last-inf", 5 + Dc - 1, INF), ("nan", 6, NAN), ("neg", 7, -1.0)):
            bad(f"sd-{tag}", fam, rh._with(b, q, v), "prior sds must be finite and > 0")
        if fam >= 2:
            bad("m_tau-nan", fam, rh._with(b, 5 + Dc, NAN), "m_tau must be finite")
            bad("m_tau-inf", fam, rh._with(b, 5 + Dc, -INF), "m_tau must be finite")
            bad("s_tau-zero", fam, rh._with(b, 6 + Dc, 0.0), "s_tau must be finite and > 0")
            bad("s_tau-inf", fam, rh._with(b, 6 + Dc, INF), "s_tau must be finite and > 0")
            bad("laid-out-for-0-1", fam, b[:5 + Dc] + b[7 + Dc:], "family must be 0 (bernoulli_logit) or 1 (poisson_log) "
                "for a block without m_tau, s_tau; families 2 (normal) and 3 (neg_binomial_2_log) take data = [family, n, "
                "p, intercept, flags, s_1..s_Dc, m_tau, s_tau, y_1..y_n, o, w, X]")
        ys, ymsg = {0: ((2.0, 0.5, -1.0, NAN), "bernoulli_logit needs y in {0, 1}"),
                    1: ((-1.0, 0.5, INF, NAN, 2.0 ** 54), "poisson_log needs y in {0, 1, 2, ..}"),
                    2: ((INF, -INF, NAN), "normal needs finite y"),
                    3: ((-1.0, 0.5, 2.0 ** 54, NAN), "neg_binomial_2_log needs y in {0, 1, 2, .., 2^53}")}[fam]
        for j, v in enumerate(ys):
            bad(f"y-{j}", fam, rh._with(b, y0 + j % n, v), ymsg)
        for j, v in enumerate((NAN, INF, -INF)):
            bad(f"o-{j}", fam, rh._with(b, o0 + j, v), "the offsets o must be finite")
        for j, v in enumerate((NAN, INF, -0.25)):
            bad(f"w-{j}", fam, rh._with(b, w0 + j, v), "the weights w must be finite and >= 0")
        zero = list(b)
        zero[w0:w0 + n] = [0.0] * n
        bad("w-all-zero", fam, zero, "at least one weight w must be > 0")
        out.append((f"ok-f{fam}-w-one-positive", rh._with(zero, w0 + 1, 0.5), None))
        bad("X-nan", fam, rh._with(b, ln - 1, NAN), "X must be finite")
        bad("X-inf", fam, rh._with(b, X0, -INF), "X must be finite")
    return out


# the model's Spec texts (layout, family, too big, sds), the two dispersion-family layouts, the shared refusals (intercept,
# n, p, no coefficients, m_tau, s_tau, four y texts, X) and the model's own (flags = 0, flags, o, w, all-zero w)
N_MESSAGES = 22


@pytest.fixture(scope="module")
def driver_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/regdata_driver.cpp"
    exe = os.path.join(str(tmp_path_factory.mktemp("oglm_regdata")), "regdata_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "smcnuts_amd", "csrc"),
                           os.path.join(ROOT, "tests", "regdata_driver.cpp"), "-o", exe])
    return exe


def _run(exe, cs):
    """cs: [(name, model, block, new rows or None)] -> the driver's parsed output"""
    path = os.path.join(os.path.dirname(exe), f"cases{len(cs)}.txt")
    rh.write_cases(path, cs)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"driver failed ({r.returncode}):\n{r.stderr[-4000:]}"
    res = rh.parse(r.stdout)
    assert list(res) == [c[0] for c in cs], "the driver did not print every case once"
    return res


@pytest.fixture(scope="module")
def driver_output(driver_exe):
    return _run(driver_exe, [(name, OGLM, b, None) for name, b, _ in cases()])


def test_cases_name_every_refusal_and_shape():
    cs = cases()
    assert len({name for name, _, _ in cs}) == len(cs)
    assert len({msg for _, _, msg in cs if msg}) == N_MESSAGES
    ok = {(int(b[4]), int(b[0]), int(b[2]), int(b[3]), int(b[1])) for _, b, msg in cs if msg is None}
    assert {(fl, f, p, ic, n) for fl in (1, 2, 3) for f in range(4) for p, ic in SHAPES for n in N_LIST} <= ok
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


def test_new_rows_are_spliced_behind_the_training_priors(driver_exe):
    """reg_splice for id 10: the new rows' block repeats the training header, flags included; the spliced block is the one
    smcn_ctx_create would take and repacks into its own image."""
    rng = np.random.default_rng(11)
    cs, want = [], {}
    for flags in (1, 2, 3):
        for fam in range(4):
            train = block(rng, fam, 5, 3, 1, flags)
            rows = block(rng, fam, 65, 3, 1, flags, priors=False)
            npri = 4 + (2 if fam >= 2 else 0)
            name = f"splice-fl{flags}-f{fam}"
            cs.append((name, OGLM, train, rows))
            want[name] = rows[:5] + train[5:5 + npri] + rows[5:]
            other = 3 if flags != 3 else 1
            cs.append((name + "-other-flags", OGLM, train, rh._with(rows, 4, float(other))))
            cs.append((name + "-other-p", OGLM, train, rh._with(rows, 2, 2.0)))
            cs.append((name + "-short", OGLM, train, rows[:4]))
    res = _run(driver_exe, cs)
    for name, _, train, rows in cs:
        got = res[name]
        assert got["msg"] == ""
        if name in want:
            assert got["splice"] == "", (name, got["splice"])
            full = np.array(want[name], dtype=np.float64)
            assert (got["full"].view(np.int64) == full.view(np.int64)).all(), name
            img, ints = image(full)
            assert got["msg2"] == "" and got["ints2"].tolist() == ints, name
            assert (got["vec2"].view(np.int64) == img.view(np.int64)).all(), name
        elif name.endswith("-short"):
            assert got["splice"] == "smcn_predict_set_data: the block is the model's data block without the priors"
        elif name.endswith("-other-flags"):
            assert got["splice"].startswith(f"smcn_predict_set_data: the new rows' flags must repeat the training "
                                            f"block's ({int(train[4])}: "), (name, got["splice"])
        else:
            assert got["splice"].startswith("smcn_predict_set_data: the new rows' header must repeat the training "
                                            "block's"), (name, got["splice"])


def test_flags_zero_names_the_plain_model_and_the_plain_id_is_untouched(driver_exe):
    """SMCN_MODEL_GLM's block under id 10 is refused by its length or its flags slot, never read past; under its own id
    it repacks as before (tests/test_regdata_host.py holds the parent's images)."""
    rng = np.random.default_rng(3)
    plain = rh.block(rng, rh.GLM, 1, 4, 2, 1)
    res = _run(driver_exe, [("plain-as-10", OGLM, plain, None), ("plain-as-4", rh.GLM, plain, None),
                            ("flags0", OGLM, plain[:4] + [0.0] + plain[4:], None)])
    assert res["plain-as-10"]["msg"].startswith(WHO)
    assert res["plain-as-4"]["msg"] == "" and res["plain-as-4"]["ints"][17] == 6      # RS = DP + 2
    assert res["flags0"]["msg"] == FLAGS0
